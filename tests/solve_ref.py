"""An independent reference for the node solve: plain numpy, nothing of oracle/ and nothing of the product.

A node is   Qd x - Ad' lam + qd + R w = 0,   l <= Ad x + B w <= u,   lam_i > 0 only at the lower bound, < 0 only at the upper
(z = [x; lam], the convention of problems.reduced_blocks: M = [[Qd, -Ad'], [Ad, 0]], q = [qd + R w; B w]).  GIVEN an active set
(side[i] = +1: row i at l_i, -1: at u_i, 0: inactive) the point solves the linear KKT system of the active rows; solve_reference
solves that system of the data as rounded to fp64, in np.longdouble (64-bit significand: a float64 LU plus iterative refinement
with longdouble residuals), and `certificate` then PROVES the point: with sym(Qd) positive definite the node is strongly
monotone and has one solution x, and a point whose active multipliers carry their side's sign and whose inactive rows are
feasible is it (its multipliers are the only ones when the rows on a bound are linearly independent: checked too).  The truth therefore does not depend on where the hint came from -- a plant, or some solver's active set.

expected_masks restates the three conditions of src/avi_solutions.jl:543-549 (tol 1e-2) on the truth; mask_safe tells where
an error of the size the accuracy bar allows cannot move a row across one of their thresholds.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla

LD = np.longdouble
EPS = 2.0 ** -52
RESID_BOUND = 2.0 ** -60          # refinement residual, relative to |rhs|_inf
WEAK_SLACK = 2.0 ** -40           # feasibility slack of the certificate, relative to the row's scale
FACTOR = 16                       # a kernel may be this many times worse than the CPU oracle on the same cases ...
FLOOR = 64 * EPS                  # ... or this far from the truth, whichever is larger
MASK_TOL = 1e-2                   # comp_indices' tol (src/avi_solutions.jl:511)
MASK_NEAR, MASK_FAR = 2e-3, 5e-2  # mask_safe: a compared quantity is either this close to its nominal value or this far beyond the threshold


def _ld(a):
    return np.asarray(a, dtype=LD)


def constraint_values(A, B, x, w):
    """a = Ad x + B w in longdouble."""
    return _ld(A) @ _ld(x) + (_ld(B) @ _ld(w) if np.size(w) else LD(0))


def stationarity(Q, R, qd, A, x, lam, w):
    """Qd x - Ad' lam + qd + R w in longdouble."""
    r = _ld(Q) @ _ld(x) + _ld(qd) + (_ld(R) @ _ld(w) if np.size(w) else LD(0))
    return r - _ld(A).T @ _ld(lam) if A.shape[0] else r


def kkt_system(Q, R, qd, A, B, l, u, w, side):
    """K = [[Qd, -A_act'], [A_act, 0]] and its right-hand side (longdouble) for the active rows of `side`."""
    side = np.asarray(side)
    rows = np.flatnonzero(side)
    n, k = Q.shape[0], rows.size
    K = np.zeros((n + k, n + k))
    K[:n, :n] = Q
    K[:n, n:] = -A[rows].T
    K[n:, :n] = A[rows]
    bound = np.where(side[rows] > 0, l[rows], u[rows])
    assert np.all(np.isfinite(bound)), "an active side has no finite bound"
    rhs = np.empty(n + k, dtype=LD)
    rhs[:n] = -(_ld(qd) + (_ld(R) @ _ld(w) if np.size(w) else LD(0)))
    rhs[n:] = _ld(bound) - (_ld(B[rows]) @ _ld(w) if np.size(w) else LD(0))
    return K, rhs, rows


def _veltkamp(a, factor):
    c = factor * a
    hi = c - (c - a)
    return hi, a - hi


def _exact_residual(K, y, rhs):
    """rhs - K y in longdouble with exact products (K's fp64 entries split into 26 + 27 bits, y's into 32 + 32: every partial
    product fits the 64-bit significand) and a compensated sum (TwoSum): good to ~2^-64 of the RESULT, not of |K| |y|."""
    Kh, Kl = _veltkamp(np.asarray(K, dtype=np.float64), 2.0 ** 27 + 1)
    yh, yl = _veltkamp(_ld(y), LD(2) ** 32 + 1)
    Kh, Kl = _ld(Kh), _ld(Kl)
    s = _ld(rhs).copy()
    c = np.zeros_like(s)
    for j in range(K.shape[1]):
        for t in (-Kh[:, j] * yh[j], -Kh[:, j] * yl[j], -Kl[:, j] * yh[j], -Kl[:, j] * yl[j]):
            v = s + t
            b = v - s
            c += (s - (v - b)) + (t - b)
            s = v
    return s + c


def refined_solve(K, rhs):
    """K y = rhs for the fp64 matrix K and the longdouble rhs: a float64 LU plus iterative refinement with longdouble residuals
    -> (y as longdouble, its residual over |rhs|_inf: at most RESID_BOUND, asserted)."""
    Kl = _ld(K)
    lu = sla.lu_factor(K)
    y = _ld(sla.lu_solve(lu, np.asarray(rhs, dtype=np.float64)))
    scale = max(float(np.max(np.abs(rhs))), np.finfo(np.float64).tiny)
    best, best_r = y, np.inf
    for _ in range(40):                                   # refine until the longdouble residual stops falling
        r = rhs - Kl @ y
        rn = float(np.max(np.abs(r))) / scale
        if rn >= best_r:
            break
        best, best_r = y, rn
        y = y + _ld(sla.lu_solve(lu, np.asarray(r, dtype=np.float64)))
    if best_r > RESID_BOUND:
        # |y| >> |rhs| (cancellation in K y): the longdouble matrix-vector product's own rounding, ~2^-64 |K| |y|, is then above
        # the bound; go on with a residual whose products are exact and whose sum is compensated
        y = best
        for _ in range(10):
            r = _exact_residual(K, y, rhs)
            rn = float(np.max(np.abs(r))) / scale
            if rn >= best_r:
                break
            best, best_r = y, rn
            y = y + _ld(sla.lu_solve(lu, np.asarray(r, dtype=np.float64)))
    if best_r > RESID_BOUND:
        # still above: no longdouble vector does better once y's own representation error, 2^-64 |K| |y|, exceeds the bound; y is
        # then asked to be that vector -- a componentwise backward error within 2^-62 (forward: cond * 2^-62, far below fp64)
        r = _exact_residual(K, best, rhs)
        assert np.all(np.abs(r) <= 2.0 ** -62 * (np.abs(Kl) @ np.abs(best) + np.abs(rhs))), \
            f"refinement stalled at {best_r:.2e} |rhs| (cond {np.linalg.cond(K):.1e})"
        best_r = min(best_r, RESID_BOUND)
    assert best_r <= RESID_BOUND, f"refinement stalled at {best_r:.2e} |rhs| (cond {np.linalg.cond(K):.1e})"
    return best, best_r


def solve_reference(Q, R, qd, A, B, l, u, w, active_hint):
    """-> (z* = [x; lam] as longdouble, info).  info: resid (longdouble residual of the KKT system over |rhs|_inf), cond (cond_2 of
    the KKT matrix), min_slack (least distance of an inactive row from its bounds), min_lam (least |multiplier| of an active row),
    ok / why (the certificate's verdict)."""
    side = np.asarray(active_hint, dtype=np.int8)
    n, m = Q.shape[0], A.shape[0]
    K, rhs, rows = kkt_system(Q, R, qd, A, B, l, u, w, side)
    best, best_r = refined_solve(K, rhs)
    z = np.zeros(n + m, dtype=LD)
    z[:n] = best[:n]
    z[n + rows] = best[n:]
    ok, why, slack = certificate(z, Q, R, qd, A, B, l, u, w, side)
    lam = np.abs(np.asarray(best[n:], dtype=np.float64))
    info = dict(resid=best_r, cond=float(np.linalg.cond(K)), min_slack=slack, min_lam=float(lam.min()) if rows.size else np.inf,
                ok=ok, why=why)
    return z, info


def certificate(z, Q, R, qd, A, B, l, u, w, side):
    """Is z = [x; lam] THE solution of the node, with the active set `side`?  -> (ok, why, least slack of an inactive row).
    sym(Qd) is positive definite (Cholesky), the stationarity residual vanishes to longdouble rounding, inactive rows carry no
    multiplier and are feasible, active rows sit on their side's bound and their multipliers carry that side's sign."""
    side = np.asarray(side)
    n, m = Q.shape[0], A.shape[0]
    x, lam = _ld(z[:n]), _ld(z[n:])
    try:
        np.linalg.cholesky(0.5 * (Q + Q.T))
    except np.linalg.LinAlgError:
        return False, "sym(Qd) is not positive definite", np.nan
    act = side != 0
    if np.any(lam[~act] != 0):
        return False, "an inactive row carries a multiplier", np.nan
    if np.any(lam[act] * side[act] <= 0):
        i = int(np.flatnonzero(act)[np.argmin(lam[act] * side[act])])
        return False, f"row {i}: multiplier {float(lam[i]):+.3e} has the wrong sign for its side ({side[i]:+d})", np.nan
    mag = np.abs(_ld(Q)) @ np.abs(x) + np.abs(_ld(qd)) + (np.abs(_ld(A)).T @ np.abs(lam) if m else 0)
    r = stationarity(Q, R, qd, A, x, lam, w)
    if np.any(np.abs(r) > 2.0 ** -52 * (1 + mag)):       # (far above longdouble rounding, far below any fp64 solver's error)
        return False, f"stationarity residual {float(np.max(np.abs(r))):.2e}", np.nan
    if m == 0:
        return True, "", np.inf
    a = constraint_values(A, B, x, w)
    # the rows' scale: what a rounding of l, u or of a term of the row moves the row by
    rs = np.abs(_ld(A)) @ np.abs(x) + (np.abs(_ld(B)) @ np.abs(_ld(w)) if np.size(w) else 0) + 1
    bound = np.where(side > 0, l, u)
    off = np.abs(a[act] - _ld(bound[act]))
    if np.any(off > 2.0 ** -52 * rs[act]):
        return False, f"an active row misses its bound by {float(off.max()):.2e}", np.nan
    # Inactive rows: l <= a <= u.  The planted weakly active rows sit on their bound only up to the rounding of l (or u), so
    # feasibility is asked up to -2^-40 of the row's scale: far more than that rounding, far less than any slack a case plants.
    lo = a - _ld(l)
    hi = _ld(u) - a
    sl = np.minimum(lo, hi)[~act]
    tolr = WEAK_SLACK * rs[~act]
    if np.any(sl < -tolr):
        return False, f"an inactive row is infeasible by {float(-sl.min()):.2e}", float(sl.min())
    # (an active row between its bounds: its other side)
    other = np.where(side > 0, hi, lo)[act]
    if np.any(other < 0):
        return False, "an active row lies beyond its other bound", np.nan
    # x is unique by strong monotonicity; the multipliers are unique only if the rows on a bound (the active ones and the weakly
    # active ones) are linearly independent -- otherwise another sign-feasible lam explains the same x
    tight = act.copy()
    tight[~act] = sl <= tolr
    if tight.any() and np.linalg.matrix_rank(A[tight]) < tight.sum():
        return False, "the rows on a bound are linearly dependent: the multipliers are not unique", float(sl.min())
    return True, "", float(sl.min()) if sl.size else np.inf


def _mask_terms(z, Q, R, qd, A, B, l, u, w):
    n, m = Q.shape[0], A.shape[0]
    x, lam = _ld(z[:n]), _ld(z[n:])
    r = np.asarray(stationarity(Q, R, qd, A, x, lam, w), dtype=np.float64)
    a = np.asarray(constraint_values(A, B, x, w), dtype=np.float64) if m else np.zeros(0)
    return r, a, np.asarray(lam, dtype=np.float64)


def expected_masks(z, Q, R, qd, A, B, l, u, w, tol=MASK_TOL):
    """active[] of a solve as src/avi_solutions.jl:543-549 gives it at the truth: the n primal rows are free variables (code 2:
    inside, zero residual), the m constraint rows carry their codes in the high nibble (value Ad x + B w against l, u; the
    multiplier in the residual's place), 8 for l ~ u (:552-558)."""
    r, a, lam = _mask_terms(z, Q, R, qd, A, B, l, u, w)
    mx = np.where(np.abs(r) <= tol, 2, 0).astype(np.uint8)
    eq = (l == u) | (np.isfinite(l) & np.isfinite(u) & (np.abs(l - u) <= tol))
    with np.errstate(invalid="ignore"):
        c1 = np.isfinite(l) & (np.abs(a - l) <= tol) & (lam >= -tol)                  # :543
        c2 = (l - tol <= a) & (a <= u + tol) & (np.abs(lam) <= tol)                   # :546
        c3 = np.isfinite(u) & (np.abs(a - u) <= tol) & (lam <= tol)                   # :549
    mg = np.where(eq, 8, c1 * 1 + c2 * 2 + c3 * 4).astype(np.uint8) << 4
    return np.concatenate([mx, mg]).astype(np.uint8)


def mask_safe(z, Q, R, qd, A, B, l, u, w, tol=MASK_TOL):
    """True where expected_masks is an assertion about ANY solver within the accuracy bar: every quantity the three conditions
    compare with +-tol (|a - l|, |a - u|, a - (l - tol), (u + tol) - a, |lam|, the primal rows' residual) is either within
    MASK_NEAR (2e-3) of the value that satisfies its condition outright (the quantities are distances: the threshold itself is
    only 1e-2 away from that value) or at least MASK_FAR (5e-2) beyond the threshold."""
    r, a, lam = _mask_terms(z, Q, R, qd, A, B, l, u, w)
    if np.any(np.abs(r) > MASK_NEAR):
        return False
    fin_l, fin_u = np.isfinite(l), np.isfinite(u)
    if np.any(fin_l & fin_u & (np.abs(u - l) < tol + MASK_FAR)):          # (no row near the l ~ u test of :512 either)
        return False
    dist = np.concatenate([np.abs(a - l)[fin_l], np.abs(a - u)[fin_u], np.abs(lam)])
    if np.any((dist > MASK_NEAR) & (dist < tol + MASK_FAR)):
        return False
    inside = np.concatenate([(a - l)[fin_l], (u - a)[fin_u]])             # (:546's range test: l - tol <= a <= u + tol)
    return not np.any((inside < -MASK_NEAR) & (inside > -(tol + MASK_FAR)))


def node_error(z, zt, n, row_norm=None):
    """max |z - z*| / max(1, |z*|_inf); with row_norm (the rowscale family) the multiplier of row i counts times |Ad_i|, the
    quantity a rescaling of the row leaves alone."""
    d = np.abs(_ld(z) - _ld(zt))
    t = np.abs(_ld(zt))
    if row_norm is not None:
        d[n:] *= row_norm
        t[n:] *= row_norm
    return float(d.max() / max(LD(1), t.max())) if d.size else 0.0


def accuracy_bar(e_ref, factor=FACTOR):
    """The bar a kernel's node_error is held to, from the CPU oracle's worst node_error on the same cell and family.  16: blocked
    elimination in another summation order, reciprocals good to 10 ulp instead of 0.5."""
    return max(factor * e_ref, FLOOR)
