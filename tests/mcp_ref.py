"""An independent reference for the box-MCP entry points (qpn_solve_avi_batch, qpn_solve_mcp_csc, qpn_check_avi_batch): plain
numpy and scipy, nothing of oracle/ and nothing of the product.

The problem, per row i with r = M z + q (kind[i] = 0: STD, 1: GAVI):

    STD    r_i  _|_  l_i <= z_i <= u_i      (r_i >= 0 at z_i = l_i, <= 0 at z_i = u_i, = 0 strictly inside)
    GAVI   z_i  _|_  l_i <= r_i <= u_i      (z_i >= 0 only at r_i = l_i, <= 0 only at r_i = u_i, = 0 strictly inside)

GIVEN a state per row (STD: lower, upper, interior, free, fixed, weak; GAVI: at_l, at_u, inside, open, eq) the point solves a
linear system: the unknowns are z_i on the rows U = STD {interior, free, weak} + GAVI {at_l, at_u, eq}, the equations are the
rows U of  M z + q = t  (t = 0 on STD rows, the bound on GAVI rows), the other z_i are known (the bound on STD bound rows, 0 on
inactive GAVI rows).  solve_reference solves it for the data as rounded to fp64, in np.longdouble (solve_ref.refined_solve: a
float64 LU plus refinement with longdouble residuals), and `certificate` then PROVES the point, whatever the states' origin.

Why a certified point is THE solution: exchanging the pair (z_i, r_i) on the GAVI rows is a principal pivot transform of the
affine map z -> M z + q.  It turns the problem into a plain box-MCP in the exchanged variables, and it keeps sum_i z_i r_i --
the same pairs, some with their members renamed -- so with sym(M) positive definite the transformed map is strongly monotone
as well: (x - y)' (F(x) - F(y)) is that sum for the difference of two points, positive, and bounded below by a multiple of
|dz|^2 + |dr|^2 >= |dx|^2.  A box-MCP over a strongly monotone map has exactly one solution, so a point that satisfies every
row's conditions is it.  (A fixed STD row, l_i = u_i, has no variable: z_i is data, the map is the one of the other rows, and
positive definiteness is asked of those -- a fixed row's column of M may even be empty.)

expected_masks restates the three conditions of src/avi_solutions.jl:543-549 (tol 1e-2) on the truth, mask_safe tells where an
error of the accuracy bar's size cannot move a row across one of their thresholds, check_degree restates the violation count of
src/avi.jl:152-154, natural_residual_ld the natural-map residual; all in longdouble.
"""
from __future__ import annotations

import numpy as np

import solve_ref as SR
from solve_ref import LD, MASK_FAR, MASK_NEAR, MASK_TOL, WEAK_SLACK, _ld

STD, GAVI = 0, 1
STD_STATES = ("lower", "upper", "interior", "free", "fixed", "weak")
GAVI_STATES = ("at_l", "at_u", "inside", "open", "eq")
_UNKNOWN = ("interior", "free", "weak", "at_l", "at_u", "eq")


def _kind(kind, N):
    return np.zeros(N, dtype=np.uint8) if kind is None else np.asarray(kind, dtype=np.uint8)


def unknown_rows(state):
    """U: the rows whose z_i is an unknown (and whose row of M z + q = t is an equation)."""
    return np.flatnonzero(np.isin(np.asarray(state), _UNKNOWN))


def linear_system(M, q, l, u, kind, state):
    """-> (M_UU (fp64), t_U - q_U - M_UF z_F (longdouble), U, z_F scattered into a length-N longdouble vector)."""
    N = q.shape[0]
    kind, state = _kind(kind, N), np.asarray(state)
    zf = np.zeros(N, dtype=LD)
    for s, b in (("lower", l), ("upper", u), ("fixed", l)):
        zf[state == s] = _ld(b)[state == s]
    U = unknown_rows(state)
    t = np.zeros(N, dtype=LD)
    for s, b in (("at_l", l), ("at_u", u), ("eq", l)):
        t[state == s] = _ld(b)[state == s]
    assert np.all(np.isfinite(np.asarray(zf, dtype=np.float64))) and np.all(np.isfinite(np.asarray(t, dtype=np.float64))), \
        "an active side has no finite bound"
    rhs = t[U] - _ld(q)[U] - _ld(M[U]) @ zf
    return np.ascontiguousarray(M[np.ix_(U, U)]), rhs, U, zf


def residual_ld(M, q, z):
    """r = M z + q in longdouble."""
    return _ld(M) @ _ld(z) + _ld(q)


def solve_reference(M, q, l, u, kind, state):
    """-> (z* as longdouble, info).  info: resid (longdouble residual of the linear system over |rhs|_inf), cond (cond_2 of
    M_UU), ok / why (the certificate's verdict)."""
    K, rhs, U, z = linear_system(M, q, l, u, kind, state)
    resid, cond = 0.0, 1.0
    if U.size:
        y, resid = SR.refined_solve(K, rhs)
        z[U] = y
        cond = float(np.linalg.cond(K))
    ok, why = certificate(z, M, q, l, u, kind, state)
    return z, dict(resid=resid, cond=cond, ok=ok, why=why)


def certificate(z, M, q, l, u, kind, state):
    """Is z THE solution of the box-MCP, with the rows in the states `state`?  -> (ok, why).  sym(M) is positive definite
    (Cholesky, over the rows that are not fixed STD rows); every row is in a state of its kind and meets that state's
    conditions: equations to longdouble rounding, the signs of residuals (STD bound rows) and multipliers (active GAVI rows)
    strict, inactive quantities strictly inside their bounds, rows on a bound exactly on it; weak rows (zero residual ON a
    bound) feasible up to WEAK_SLACK of the row's scale."""
    N = q.shape[0]
    kind, state = _kind(kind, N), np.asarray(state)
    z = _ld(z)
    # (a fixed STD row's z_i = l_i = u_i is data, not a variable: the map of the problem is the one of the other rows)
    R = np.flatnonzero(~((kind == 0) & (l == u)))
    try:
        np.linalg.cholesky(0.5 * (M + M.T)[np.ix_(R, R)])
    except np.linalg.LinAlgError:
        return False, "sym(M) is not positive definite"
    r = residual_ld(M, q, z)
    mag = np.abs(_ld(M)) @ np.abs(z) + np.abs(_ld(q))
    tiny = 2.0 ** -52 * (1 + mag)                        # (far above longdouble rounding, far below any fp64 solver's error)
    ll, uu = _ld(l), _ld(u)
    for i in range(N):
        s = str(state[i])
        if s not in (GAVI_STATES if kind[i] else STD_STATES):
            return False, f"row {i}: state {s} is not one of a {'GAVI' if kind[i] else 'STD'} row"
        if not l[i] <= u[i]:
            return False, f"row {i}: l > u"
        p, d = (r[i], z[i]) if kind[i] else (z[i], r[i])       # the bounded member and its multiplier
        # the member that an equation sets is compared up to rounding, the one that is data exactly
        eqtol = tiny[i] if kind[i] else 0
        if s in ("lower", "at_l", "upper", "at_u"):
            lo = s in ("lower", "at_l")
            b, other = (ll[i], uu[i] - p) if lo else (uu[i], p - ll[i])
            if not np.isfinite(float(b)) or abs(p - b) > eqtol:
                return False, f"row {i} ({s}): misses its bound by {float(abs(p - b)):.2e}"
            if not (d > tiny[i] if lo else d < -tiny[i]):
                return False, f"row {i} ({s}): multiplier {float(d):+.3e} has the wrong sign for its side"
            if other < 0:
                return False, f"row {i} ({s}): lies beyond its other bound"
        elif s in ("fixed", "eq"):
            if l[i] != u[i] or abs(p - ll[i]) > eqtol:
                return False, f"row {i} ({s}): not on l = u"
        elif s in ("interior", "free", "inside", "open"):
            if abs(d) > (0 if kind[i] else tiny[i]):
                return False, f"row {i} ({s}): an inactive row carries a multiplier {float(d):+.3e}"
            if s in ("free", "open") and not (l[i] == -np.inf and u[i] == np.inf):
                return False, f"row {i} ({s}): has a finite bound"
            if not ll[i] + (tiny[i] if kind[i] else 0) < p < uu[i] - (tiny[i] if kind[i] else 0):
                return False, f"row {i} ({s}): infeasible or on a bound, by {float(min(p - ll[i], uu[i] - p)):.2e}"
        else:                                                   # weak
            if abs(d) > tiny[i]:
                return False, f"row {i} (weak): residual {float(d):+.3e}"
            slack = WEAK_SLACK * (1 + abs(p))
            on = min(abs(p - ll[i]), abs(p - uu[i]))
            if on > slack or p < ll[i] - slack or p > uu[i] + slack:
                return False, f"row {i} (weak): not on a bound, by {float(on):.2e}"
    return True, ""


def _pd(M, q, kind, z):
    N = q.shape[0]
    g = _kind(kind, N).astype(bool)
    z = _ld(z)
    r = residual_ld(M, q, z)
    return np.where(g, r, z), np.where(g, z, r), g, r


def expected_masks(z, M, q, l, u, kind, tol=MASK_TOL):
    """active[] of a solve as src/avi_solutions.jl:543-549 gives it at z: the three conditions on (p, d) = (z, r) for STD rows
    (low nibble) and (r, z) for GAVI rows (high nibble), 8 for l ~ u (:552-558)."""
    p, d, g, _ = _pd(M, q, kind, z)
    p, d = np.asarray(p, dtype=np.float64), np.asarray(d, dtype=np.float64)
    eq = (l == u) | (np.isfinite(l) & np.isfinite(u) & (np.abs(l - u) <= tol))
    with np.errstate(invalid="ignore"):
        c1 = np.isfinite(l) & (np.abs(p - l) <= tol) & (d >= -tol)                    # :543
        c2 = (l - tol <= p) & (p <= u + tol) & (np.abs(d) <= tol)                     # :546
        c3 = np.isfinite(u) & (np.abs(p - u) <= tol) & (d <= tol)                     # :549
    m = np.where(eq, 8, c1 * 1 + c2 * 2 + c3 * 4).astype(np.uint8)
    return np.where(g, m << 4, m).astype(np.uint8)


def mask_safe(z, M, q, l, u, kind, tol=MASK_TOL):
    """True where expected_masks is an assertion about ANY solver within the accuracy bar: every quantity the three conditions
    compare with +-tol is either within MASK_NEAR of the value that satisfies its condition outright or at least MASK_FAR beyond
    the threshold (solve_ref.mask_safe, on the pairs (p, d) of this problem)."""
    p, d, _, _ = _pd(M, q, kind, z)
    p, d = np.asarray(p, dtype=np.float64), np.asarray(d, dtype=np.float64)
    fin_l, fin_u = np.isfinite(l), np.isfinite(u)
    if np.any(fin_l & fin_u & (l != u) & (np.abs(u - l) < tol + MASK_FAR)):
        return False
    ne = l != u                                                                       # (rows with l = u carry 8 whatever p, d)
    dist = np.concatenate([np.abs(p - l)[fin_l & ne], np.abs(p - u)[fin_u & ne], np.abs(d)[ne]])
    if np.any((dist > MASK_NEAR) & (dist < tol + MASK_FAR)):
        return False
    inside = np.concatenate([(p - l)[fin_l & ne], (u - p)[fin_u & ne]])
    return not np.any((inside < -MASK_NEAR) & (inside > -(tol + MASK_FAR)))


def natural_residual_ld(M, q, l, u, kind, z):
    """max_k |p - clip(p - d, l, u)| in longdouble."""
    p, d, _, _ = _pd(M, q, kind, z)
    return (np.abs(p - np.minimum(np.maximum(p - d, _ld(l)), _ld(u)))).max()


def matvec_bound(M, q, z):
    """gamma = 2 N eps max_i (|M| |z| + |q|)_i: the rounding bound of an N-term fma sum per row (with room for the order)."""
    N = q.shape[0]
    return 2 * N * SR.EPS * float((np.abs(M) @ np.abs(np.asarray(z, dtype=np.float64)) + np.abs(q)).max())


def check_degree(M, q, l, u, kind, z, tol=1e-6):
    """The violation count of src/avi.jl:152-154 in longdouble -> (degree, per-row flags: bit 0 d > tol off l, bit 1 d < -tol off
    u, bit 2 p < l - tol, bit 3 p > u + tol, bit 4 NaN; margin: the least distance of a compared quantity from its threshold)."""
    p, d, _, _ = _pd(M, q, kind, z)
    ll, uu = _ld(l), _ld(u)
    with np.errstate(invalid="ignore"):
        f = ((d > tol) & (np.abs(p - ll) > tol)) * 1 + ((d < -tol) & (np.abs(p - uu) > tol)) * 2 + (p - ll < -tol) * 4 + \
            (p - uu > tol) * 8 + (np.isnan(p) | np.isnan(d)) * 16
        cmp = np.concatenate([np.abs(d), np.abs(p - ll), np.abs(p - uu)])
        cmp = cmp[np.isfinite(np.asarray(cmp, dtype=np.float64))]
    margin = float(np.abs(cmp - tol).min()) if cmp.size else np.inf
    f = np.asarray(f, dtype=np.int64)
    return int(sum(bin(int(v)).count("1") for v in f)), f, margin


def mcp_error(z, zt):
    """max |z - z*| / max(1, |z*|_inf)."""
    d = np.abs(_ld(z) - _ld(zt))
    return float(d.max() / max(LD(1), np.abs(_ld(zt)).max())) if d.size else 0.0
