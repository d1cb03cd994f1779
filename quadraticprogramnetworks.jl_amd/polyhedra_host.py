"""The numpy twins of the polyhedral entries, the normative statements of the kernels' methods (the kernels are bit-equal to them):
solve_lps_host, issubset_pairs_host, implicit_bounds_host, irredundant_bounds_host, exemplar_polys_host, exemplar_products_host, intersection_trees_host, interior_member_records, members_outside_host and members_outside_lists_host,
with the entries' result codes, defined here once (_lib.py and polyhedra.py import them).  Numpy alone, loadable as a stand-alone
file: tests/golden/lp_twin_record.json pins it across commits.  The front ends that pack, route and call an engine are polyhedra.py.
"""
from __future__ import annotations

import numpy as np

INF = np.inf


# ---- the LP solver (qpn_solve_lps): bounded-variable primal simplex, the numpy twin -----------------------------------------
LP_OPTIMAL, LP_INFEASIBLE, LP_UNBOUNDED, LP_ITER_LIMIT, LP_FAILURE = 1, 2, 3, 4, 5
LP_PIV_BAND = 1.0 - 2.0 ** -30                  # pivot / pricing candidates within this factor of the best count as equal
LP_RATIO_TIE = 1e-12                            # ratios within this (relative, at least absolute) of the smallest count as tied
LP_BLAND_AFTER = 20                             # consecutive zero-length steps before the lowest eligible id enters
LP_DEFAULT_OPTS = dict(piv_tol=1e-9, feas_tol=1e-9, opt_tol=1e-9, check_tol=1e-6, max_iters=0)
LP_MAX_D, LP_MAX_R = 256, 1024


def _lp_pivot(T, i, j):
    """Exchange the basic variable of row i and the nonbasic one of column j of the dictionary T [r + 1, d] (cost row last)."""
    p = T[i, j]
    col = T[:, j].copy()
    new = -T[i, :] / p
    new[j] = 1.0 / p
    T += col[:, None] * new[None, :]
    T[:, j] = col / p
    T[i, :] = new


class _LpState:
    """What a solve leaves for the next one over the same polyhedron: the dictionary T [r + 1, d] (cost row last), the ids of the
    basic (rb) and nonbasic (cn) variables, the nonbasic values xn; and what the last loop left for the check (xb, g, dj, e, dirn, a)."""


def _lp_setup(A, l, u, c, o):
    """Steps 0-4 of qpn_solve_lps: the data screen, scaling, the dictionary, the crash, the nonbasic values.  -> _LpState; S.nonfinite
    is set when step 0 fails the job; S.zbad is the all-zero row outside its bounds that settles the job (its unit Farkas vector in
    S.zlam), or None."""
    r, d = A.shape
    S = _LpState()
    S.A, S.l, S.u, S.r, S.d, S.o = A, l, u, r, d, o
    S.max_iters = o["max_iters"] if o["max_iters"] > 0 else 50 * (r + d) + 100
    S.zbad, S.iters, S.e, S.dirn, S.a, S.g, S.dj, S.xb = None, 0, -1, 0.0, None, None, None, np.zeros(r)
    piv_tol = o["piv_tol"]
    with np.errstate(all="ignore"):
        # 0. the data screen: an entry of A or c that is not finite, a bound that is not a number, l = +inf or u = -inf
        S.nonfinite = not bool(np.all(np.abs(A) < INF) and np.all(np.abs(c) < INF) and np.all(l < INF) and np.all(u > -INF))
        if S.nonfinite:
            return S
        # 1. row scaling; an all-zero row outside its bounds settles the job
        amax = np.max(np.abs(A), axis=1)
        S.amax = amax
        for i in range(r):
            if amax[i] == 0.0 and (u[i] < 0.0 or l[i] > 0.0):
                S.zbad = i
                S.zlam = np.zeros(r)
                S.zlam[i] = 1.0 if u[i] < 0.0 else -1.0
                return S
        sc = np.ones(r)
        nz = amax > 0.0
        sc[nz] = 1.0 / amax[nz]
        ls, us = l * sc, u * sc
        # 2. the dictionary: basic = T nonbasic, the cost row below it
        T = np.empty((r + 1, d))
        T[:r] = A * sc[:, None]
        T[r] = c
        rb = d + np.arange(r); cn = np.arange(d)
        # 3. crash: the x come into the basis, column by column
        for j in range(d):
            col = np.where(rb >= d, np.abs(T[:r, j]), 0.0)
            best = np.max(col)
            if not best > piv_tol:
                continue
            i = int(np.nonzero((rb >= d) & (col >= best * LP_PIV_BAND))[0][0])
            _lp_pivot(T, i, j)
            rb[i], cn[j] = cn[j], rb[i]
        # 4. nonbasic values
        xn = np.zeros(d)
        for j in range(d):
            if cn[j] >= d:
                lo, hi = ls[cn[j] - d], us[cn[j] - d]
                if np.isfinite(lo) and np.isfinite(hi):
                    xn[j] = lo if abs(lo) <= abs(hi) else hi
                elif np.isfinite(lo):
                    xn[j] = lo
                elif np.isfinite(hi):
                    xn[j] = hi
    S.sc, S.ls, S.us, S.T, S.rb, S.cn, S.xn = sc, ls, us, T, rb, cn, xn
    return S


def _lp_loop(S, iters0=0):
    """Steps 5-8: the simplex loop from the state's dictionary, with a fresh degeneracy counter and the step counter at iters0 (the
    steps of the loop before a rebuild count against the same max_iters).  -> status; the steps in S.iters, the basic values,
    violations and reduced costs of the last round in S.xb, S.g, S.dj, the last entering column and direction in S.e, S.dirn, S.a."""
    r, d, T, rb, cn, xn, ls, us = S.r, S.d, S.T, S.rb, S.cn, S.xn, S.ls, S.us
    piv_tol, feas_tol, opt_tol, max_iters = S.o["piv_tol"], S.o["feas_tol"], S.o["opt_tol"], S.max_iters
    with np.errstate(all="ignore"):
        status, iters, degen = LP_FAILURE, iters0, 0
        e, dirn, a, g, dj = -1, 0.0, None, None, None
        while True:
            lob = np.where(rb >= d, ls[np.maximum(rb - d, 0)], -INF); upb = np.where(rb >= d, us[np.maximum(rb - d, 0)], INF)
            lon = np.where(cn >= d, ls[np.maximum(cn - d, 0)], -INF); upn = np.where(cn >= d, us[np.maximum(cn - d, 0)], INF)
            xb = np.zeros(r)
            for j in range(d):                          # (a nonbasic at 0 adds nothing)
                if xn[j] != 0.0:
                    xb = xb + T[:r, j] * xn[j]
            below = xb < lob - feas_tol * np.maximum(1.0, np.abs(lob))
            above = xb > upb + feas_tol * np.maximum(1.0, np.abs(upb))
            g = np.where(below, -1.0, np.where(above, 1.0, 0.0))
            phase1 = bool(np.any(g != 0.0))
            if phase1:                                  # 5. the gradient of the sum of violations
                dj = np.zeros(d)
                for i in range(r):
                    if g[i] != 0.0:
                        dj = dj + g[i] * T[i, :]
            else:
                dj = T[r].copy()
            # 6. the entering variable
            free = lon != upn
            inc = (dj < -opt_tol) & (xn < upn) & free
            dec = (dj > opt_tol) & (xn > lon) & free
            elig = inc | dec
            if not elig.any():
                status = LP_INFEASIBLE if phase1 else LP_OPTIMAL
                break
            if degen >= LP_BLAND_AFTER:
                pick = elig
            else:
                mag = np.where(elig, np.abs(dj), 0.0)
                pick = elig & (mag >= np.max(mag) * LP_PIV_BAND)
            e = int(np.argmin(np.where(pick, cn, r + d)))
            dirn = 1.0 if inc[e] else -1.0
            # 7. the ratio test
            a = T[:r, e] * dirn
            tgt = np.where(a > 0.0, np.where(below, lob, np.where(above, INF, upb)), np.where(above, upb, np.where(below, -INF, lob)))
            ratio = np.where(np.abs(a) > piv_tol, np.maximum((tgt - xb) / a, 0.0), INF)
            tflip = upn[e] - xn[e] if dirn > 0.0 else xn[e] - lon[e]
            tmin = min(tflip, np.min(ratio)) if r else tflip
            if not tmin < INF:
                status = LP_FAILURE if phase1 else LP_UNBOUNDED
                break
            thr = tmin + LP_RATIO_TIE * max(1.0, tmin)
            win = int(np.min(np.where(ratio <= thr, rb, r + d))) if r else r + d
            if tflip <= thr and cn[e] < win:
                win = int(cn[e])
            if win == r + d:                            # (not-a-number data: no candidate compares)
                status = LP_FAILURE
                break
            if iters >= max_iters:                      # a step is due and none is left: a job that ends within max_iters keeps its outcome
                status = LP_ITER_LIMIT
                break
            iters += 1
            degen = degen + 1 if tmin == 0.0 else 0
            if win == cn[e]:
                xn[e] = upn[e] if dirn > 0.0 else lon[e]
            else:
                i = int(np.nonzero(rb == win)[0][0])
                _lp_pivot(T, i, e)                      # 8.
                rb[i], cn[e] = cn[e], rb[i]
                xn[e] = tgt[i]
    S.iters, S.e, S.dirn, S.a, S.g, S.dj, S.xb = iters, e, dirn, a, g, dj, xb
    return status


def _lp_point(S, c):
    """Step 9, first half: the point the loop ended at, on the unscaled data.  -> (x [d], obj = c'x)."""
    x = np.zeros(S.d)
    with np.errstate(all="ignore"):
        for j in range(S.d):
            if S.cn[j] < S.d:
                x[S.cn[j]] = S.xn[j]
        for i in range(S.r):
            if S.rb[i] < S.d:
                x[S.rb[i]] = S.xb[i]
        obj = 0.0
        for k in range(S.d):
            obj = obj + c[k] * x[k]
    return x, obj


def _lp_check(S, status, c, x):
    """Step 9, second half: the check of what an OPTIMAL / UNBOUNDED / INFEASIBLE end claims, on the unscaled data at check_tol.
    -> (ok, lambda [r], ray [d])."""
    A, l, u, r, d, rb, cn, sc, amax = S.A, S.l, S.u, S.r, S.d, S.rb, S.cn, S.sc, S.amax
    ct = S.o["check_tol"]
    e, dirn, a, g, dj = S.e, S.dirn, S.a, S.g, S.dj
    lam = np.zeros(r); ray = np.zeros(d)
    with np.errstate(all="ignore"):
        s = np.zeros(r)
        for j in range(d):
            s = s + A[:, j] * x[j]
        tl = ct * np.maximum(1.0, np.abs(l)); tu = ct * np.maximum(1.0, np.abs(u))
        ok = True
        if status != LP_INFEASIBLE:
            ok = bool(np.all((s >= l - tl) & (s <= u + tu)))
        if status == LP_OPTIMAL:
            for j in range(d):
                if cn[j] >= d:
                    lam[cn[j] - d] = dj[j] * sc[cn[j] - d]
            for k in range(d):
                acc = 0.0
                for i in range(r):
                    acc = acc + A[i, k] * lam[i]
                ok = ok and bool(abs(c[k] - acc) <= ct * max(1.0, abs(c[k])))
            ok = ok and bool(np.all(~(lam > ct) | (np.abs(s - l) <= tl)) and np.all(~(lam < -ct) | (np.abs(s - u) <= tu)))
        elif status == LP_UNBOUNDED:
            if cn[e] < d:
                ray[cn[e]] = dirn
            for i in range(r):
                if rb[i] < d:
                    ray[rb[i]] = a[i]
            cr = 0.0
            for k in range(d):
                cr = cr + c[k] * ray[k]
            ar = np.zeros(r)
            for j in range(d):
                ar = ar + A[:, j] * ray[j]
            tr = ct * max(1.0, float(np.max(np.abs(ray)))) * amax
            ok = ok and bool(cr < 0.0) and bool(np.all(~np.isfinite(l) | (ar >= -tr)) and np.all(~np.isfinite(u) | (ar <= tr)))
        else:
            for i in range(r):
                if rb[i] >= d:
                    lam[rb[i] - d] = g[i] * sc[rb[i] - d]
            for j in range(d):
                if cn[j] >= d:
                    k = cn[j] - d
                    y = -dj[j]
                    if (y > 0.0 and not np.isfinite(u[k])) or (y < 0.0 and not np.isfinite(l[k])):
                        y = 0.0
                    lam[k] = y * sc[k]
            ymax = max(1.0, float(np.max(np.abs(lam)))) if r else 1.0
            for k in range(d):
                acc = 0.0
                for i in range(r):
                    acc = acc + A[i, k] * lam[i]
                ok = ok and bool(abs(acc) <= ct * ymax)
            # the Farkas sum is negative by more than every bound relaxed by the tolerance primal feasibility is judged at accounts for
            bound, slack = 0.0, 0.0
            for i in range(r):
                if lam[i] > 0.0:
                    bound = bound + lam[i] * u[i]
                    slack = slack + lam[i] * tu[i]
                elif lam[i] < 0.0:
                    bound = bound + lam[i] * l[i]
                    slack = slack - lam[i] * tl[i]
            ok = ok and bool(bound < -slack)
    return ok, lam, ray


def _lp_rebuild(S, c):
    """The dictionary of the current basis once more from the scaled rows (step 10): T = A * sc with the cost row c, every x
    nonbasic; then, for the columns j ascending whose x is basic in the current basis (a row's id stands in column j), the crash's
    pivot restricted to the rows whose id is nonbasic in the current basis and still basic here: the largest |T[i, j]|, the lowest
    i within PIV_BAND of it.  At most d pivots.  The nonbasic rows keep their values.  -> False when a pivot is not above piv_tol."""
    r, d, T, rb, cn, xn = S.r, S.d, S.T, S.rb, S.cn, S.xn
    with np.errstate(all="ignore"):
        out = np.zeros(r, bool); val = np.zeros(r)
        for j in range(d):
            if cn[j] >= d:
                out[cn[j] - d] = True; val[cn[j] - d] = xn[j]
        want = cn >= d                                  # (a nonbasic x never left its own column)
        T[:r] = S.A * S.sc[:, None]
        T[r] = c
        rb[:] = d + np.arange(r); cn[:] = np.arange(d)
        for j in range(d):
            if not want[j]:
                continue
            cand = out & (rb >= d)
            col = np.where(cand, np.abs(T[:r, j]), 0.0)
            best = np.max(col)
            if not best > S.o["piv_tol"]:
                return False
            i = int(np.nonzero(cand & (col >= best * LP_PIV_BAND))[0][0])
            _lp_pivot(T, i, j)
            rb[i], cn[j] = cn[j], rb[i]
        for j in range(d):
            if cn[j] >= d:
                xn[j] = val[cn[j] - d]
    return True


def _lp_finish(S, c, cold):
    """Steps 5-10 from the state's dictionary: the loop, the point and step 9's check; an end that is not certified -- a FAILURE of
    the loop, an INFEASIBLE end of a warm solve (the polyhedron has a point), a certificate that fails -- rebuilds the dictionary
    (_lp_rebuild) and runs the loop once more, the step counter going on; what that ends with stands.  cold: an INFEASIBLE end is
    an outcome (checked like the others), and with cold == "feasible" an OPTIMAL end is taken unchecked (c = 0: lp_feasible).
    -> (status, x, obj, lambda, ray); every status but a certified one comes with lambda = ray = 0."""
    r, d = S.r, S.d
    iters0 = 0
    for attempt in (0, 1):
        status = _lp_loop(S, iters0)
        iters0 = S.iters
        x, obj = _lp_point(S, c)
        if status == LP_ITER_LIMIT:
            return status, x, obj, np.zeros(r), np.zeros(d)
        if status == LP_OPTIMAL and cold == "feasible":
            return status, x, obj, np.zeros(r), np.zeros(d)
        if status in (LP_OPTIMAL, LP_UNBOUNDED) or (status == LP_INFEASIBLE and cold):
            ok, lam, ray = _lp_check(S, status, c, x)
            if ok:
                return status, x, obj, lam, ray
        if attempt == 1 or not _lp_rebuild(S, c):
            break
    return LP_FAILURE, x, obj, np.zeros(r), np.zeros(d)


def _lp_one(A, l, u, c, o):
    """One LP  min c'x  s.t.  l <= A x <= u  (A [r, d] math layout) by the method of qpn_solve_lps (include/qpn_hip.h states it):
    set-up, then loop, check and at most one rebuild (_lp_finish) -- the parts issubset_pairs_host runs too.
    -> (status, x [d], obj, lambda [r], ray [d], iters)."""
    S = _lp_setup(A, l, u, c, o)
    if S.nonfinite:
        return LP_FAILURE, np.zeros(S.d), 0.0, np.zeros(S.r), np.zeros(S.d), 0
    if S.zbad is not None:
        return LP_INFEASIBLE, np.zeros(S.d), 0.0, S.zlam, np.zeros(S.d), 0
    status, x, obj, lam, ray = _lp_finish(S, c, True)
    return status, x, obj, lam, ray, S.iters


def _lp_feasible(A, l, u, o):
    """The feasibility solve of issubset_pairs_host (a) and implicit_bounds_host (a) (the kernel's lp_feasible): steps 0-8 and 10
    with c = 0.  Data the screen rejects is LP_FAILURE at 0 steps; an infeasible all-zero row, or an INFEASIBLE end whose Farkas
    certificate holds, is LP_INFEASIBLE; one whose certificate fails after the rebuild too LP_FAILURE.
    -> (LP_OPTIMAL / LP_INFEASIBLE / LP_ITER_LIMIT / LP_FAILURE, S, x [d]); the steps in S.iters."""
    zero = np.zeros(A.shape[1])
    S = _lp_setup(A, l, u, zero, o)
    if S.nonfinite:
        return LP_FAILURE, S, zero
    if S.zbad is not None:
        return LP_INFEASIBLE, S, zero
    status, x, _, _, _ = _lp_finish(S, zero, "feasible")
    return status, S, x


def _lp_resolve(S, c):
    """The solve of objective c from the basis the previous solve over the polyhedron left (the kernel's lp_resolve): the cost
    row of c in the current dictionary (issubset_pairs_host (e)), then _lp_finish: the loop with fresh step and degeneracy counters,
    the point, step 9's check and, where the end is not certified, the rebuild and the loop once more.  -> (LP_OPTIMAL or
    LP_UNBOUNDED, certified / LP_ITER_LIMIT / LP_FAILURE: a FAILURE of the loop, an INFEASIBLE end, a certificate that fails, after
    the rebuild too; x [d]; obj = c'x); the steps in S.iters."""
    T, rb, cn, r, d = S.T, S.rb, S.cn, S.r, S.d
    with np.errstate(all="ignore"):
        row = np.zeros(d)
        for i in range(r):
            if rb[i] < d:
                row = row + c[rb[i]] * T[i, :]
        for j in range(d):
            if cn[j] < d:
                row[j] = row[j] + c[cn[j]]
        T[r] = row
    status, x, obj, _, _ = _lp_finish(S, c, False)
    return status, x, obj


def solve_lps_host(Ac, l, u, poly_of, cost=None, obj_row=None, obj_sign=None, opts=None):
    """The numpy twin of Engine.solve_lps (qpn_solve_lps), the normative statement of the method: the kernel does the same
    operations in the same order (every sum over the ascending index as acc = acc + a * b, no contraction), so every output is
    bit-equal.  Ac [polys, d, r] (the polyhedra's matrices in the ABI layout), l, u [polys, r] (+-inf allowed), poly_of [jobs];
    the objective of job t is cost[t] or, without `cost`, obj_sign[t] * row obj_row[t] of its polyhedron.
    -> dict(status [jobs] int32, x [jobs, d], obj [jobs], lam [jobs, r], ray [jobs, d], iters [jobs] int32).  A job whose
    poly_of / obj_row is out of range answers LP_FAILURE with zeros (the kernel's rule for device index arrays), and so does one
    whose data the screen of step 0 rejects; every LP_FAILURE and LP_ITER_LIMIT has lam = ray = 0."""
    Ac = np.asarray(Ac, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    polys, d, r = Ac.shape
    poly_of = np.asarray(poly_of, dtype=np.int64)
    jobs = len(poly_of)
    o = dict(LP_DEFAULT_OPTS)
    o.update(opts or {})
    out = dict(status=np.zeros(jobs, np.int32), x=np.zeros((jobs, d)), obj=np.zeros(jobs), lam=np.zeros((jobs, r)),
               ray=np.zeros((jobs, d)), iters=np.zeros(jobs, np.int32))
    for t in range(jobs):
        b = int(poly_of[t])
        row_ok = cost is not None or 0 <= int(obj_row[t]) < r
        if not (0 <= b < polys) or not row_ok:
            out["status"][t] = LP_FAILURE
            continue
        A = np.ascontiguousarray(Ac[b].T)
        c = np.asarray(cost[t], dtype=np.float64) if cost is not None else float(obj_sign[t]) * A[int(obj_row[t])]
        st, x, obj, lam, ray, it = _lp_one(A, l[b], u[b], c, o)
        out["status"][t] = st; out["x"][t] = x; out["obj"][t] = obj; out["lam"][t] = lam; out["ray"][t] = ray; out["iters"][t] = it
    return out


# ---- subset tests (qpn_issubset_pairs): one job per pair, the numpy twin ---------------------------------------------------------
SUBSET_HOLDS, SUBSET_BY_POINT, SUBSET_BY_OPTIMUM, SUBSET_UNBOUNDED, SUBSET_ITER_LIMIT, SUBSET_FAILURE, SUBSET_EMPTY = 0, 1, 2, 3, 4, 5, 6


def _subset_one(A1, l1, u1, A2, l2, u2, tol, o):
    """One pair P1 ⊆ P2 by the method of qpn_issubset_pairs (A1 [r1, d], A2 [r2, d] math layout).
    -> (how, bound, val, lps, iters)."""
    d = A1.shape[1]
    # (a) the feasibility solve: steps 1-8 with c = 0
    status, S, x = _lp_feasible(A1, l1, u1, o)
    lps, iters = 1, S.iters
    if status != LP_OPTIMAL:
        return {LP_INFEASIBLE: SUBSET_EMPTY, LP_ITER_LIMIT: SUBSET_ITER_LIMIT}.get(status, SUBSET_FAILURE), -1, 0.0, lps, iters
    with np.errstate(all="ignore"):
        for i in range(A2.shape[0]):                        # (b) the bounds in order, the lower before the upper
            fl, fu = bool(np.abs(l2[i]) < INF), bool(np.abs(u2[i]) < INF)
            if not (fl or fu):
                continue
            # (c) rows of P1 equal to this one: the tightest of their bounds
            same = np.all(A1 == A2[i][None, :], axis=1)
            lo1, hi1 = -INF, INF
            for k in range(A1.shape[0]):
                if same[k]:
                    lo1 = max(lo1, l1[k]) if l1[k] == l1[k] else lo1
                    hi1 = min(hi1, u1[k]) if u1[k] == u1[k] else hi1
            for side in (0, 1):
                if side == 0:
                    if not fl or lo1 >= l2[i] - tol:
                        continue
                    c, beta = A2[i].copy(), l2[i]
                else:
                    if not fu or hi1 <= u2[i] + tol:
                        continue
                    c, beta = -A2[i], -u2[i]
                b = 2 * i + side
                # (d) the point the previous solve ended at
                v = 0.0
                for k in range(d):
                    v = v + c[k] * x[k]
                if v < beta - tol:
                    return SUBSET_BY_POINT, b, v, lps, iters
                # (e) the cost row of c in the current dictionary, (f) solve and decide
                lps += 1
                status, x, obj = _lp_resolve(S, c)
                iters += S.iters
                if status == LP_ITER_LIMIT:
                    return SUBSET_ITER_LIMIT, b, 0.0, lps, iters
                if status == LP_FAILURE:
                    return SUBSET_FAILURE, b, 0.0, lps, iters
                if status == LP_UNBOUNDED:
                    return SUBSET_UNBOUNDED, b, 0.0, lps, iters
                if obj < beta - tol:
                    return SUBSET_BY_OPTIMUM, b, obj, lps, iters
    return SUBSET_HOLDS, -1, 0.0, lps, iters                # (g)


def issubset_pairs_host(A1c, l1, u1, A2c, l2, u2, pi, pj, tol=1e-6, opts=None):
    """The numpy twin of Engine.issubset_pairs (qpn_issubset_pairs), the normative statement of the method; every output of the
    kernel is bit-equal to it.  Pair q asks whether first piece pi[q] ⊆ second piece pj[q].  A1c [B1, d, r1], A2c [B2, d, r2]
    (ABI layout), l1, u1 [B1, r1], l2, u2 [B2, r2] (+-inf allowed).

    (a) solve_lps_host's steps 1-8 on P1 with c = 0 (the crash and phase 1, once per pair; _lp_feasible); an INFEASIBLE end whose Farkas
    certificate holds is EMPTY (sub = 1, the convention of issubset_batch), otherwise FAILURE.  (b) the rows of P2 ascending, the
    lower bound (c = +a, beta = l2) before the upper (c = -a, beta = -u2), non-finite bounds skipped.  (c) a bound is skipped
    when rows of P1 equal the row of P2 entry by entry (==, unscaled) and the largest of their l1 is >= l2 - tol (the smallest of
    their u1 is <= u2 + tol).  (d) v = c'x at the point the previous solve ended at: v < beta - tol is BY_POINT.  (e) the cost
    row of c in the current dictionary: column j, acc = 0, over the rows i ascending with an x basic acc = acc + c[rb[i]] * T[i, j],
    then + c[cn[j]] when an x is nonbasic there.  (f) the loop with fresh step and degeneracy counters, step 9's check on P1
    ((e) and (f) are _lp_resolve):
    OPTIMAL with obj < beta - tol is BY_OPTIMUM, a certified ray UNBOUNDED, a failed certificate or an INFEASIBLE end that the
    rebuild and the second loop of _lp_finish do not mend FAILURE, ITER_LIMIT / FAILURE themselves.  (g) no bound left: HOLDS.
    -> dict(sub [pairs] uint8, how [pairs] int32 (SUBSET_*), bound [pairs] int32 (2 i + side of the deciding bound, -1 without),
    val [pairs] (the value that decided: BY_POINT, BY_OPTIMUM), lps [pairs] int32 (solves started, the feasibility solve counted),
    iters [pairs] int32 (all steps)).  A pair whose pi / pj is out of range answers FAILURE with bound -1 and zeros (the kernel's
    rule for device index arrays)."""
    A1c = np.asarray(A1c, dtype=np.float64); l1 = np.asarray(l1, dtype=np.float64); u1 = np.asarray(u1, dtype=np.float64)
    A2c = np.asarray(A2c, dtype=np.float64); l2 = np.asarray(l2, dtype=np.float64); u2 = np.asarray(u2, dtype=np.float64)
    B1, B2 = A1c.shape[0], A2c.shape[0]
    pi = np.asarray(pi, dtype=np.int64); pj = np.asarray(pj, dtype=np.int64)
    n = len(pi)
    o = dict(LP_DEFAULT_OPTS)
    o.update(opts or {})
    out = dict(sub=np.zeros(n, np.uint8), how=np.zeros(n, np.int32), bound=np.full(n, -1, np.int32), val=np.zeros(n),
               lps=np.zeros(n, np.int32), iters=np.zeros(n, np.int32))
    mats1, mats2 = {}, {}
    for q in range(n):
        a, b = int(pi[q]), int(pj[q])
        if not (0 <= a < B1 and 0 <= b < B2):
            out["how"][q] = SUBSET_FAILURE
            continue
        if a not in mats1:
            mats1[a] = np.ascontiguousarray(A1c[a].T)
        if b not in mats2:
            mats2[b] = np.ascontiguousarray(A2c[b].T)
        how, bound, val, lps, iters = _subset_one(mats1[a], l1[a], u1[a], mats2[b], l2[b], u2[b], float(tol), o)
        out["how"][q] = how; out["bound"][q] = bound; out["val"][q] = val; out["lps"][q] = lps; out["iters"][q] = iters
        out["sub"][q] = 1 if how in (SUBSET_HOLDS, SUBSET_EMPTY) else 0
    return out


# ---- implicit bounds (qpn_implicit_bounds): one job per polyhedron, the numpy twin ----------------------------------------------
IB_OK, IB_EMPTY, IB_ITER_LIMIT, IB_FAILURE = 0, 1, 2, 3
IB_HOW_UNDECIDED, IB_HOW_EXPLICIT, IB_HOW_IMPLICIT, IB_HOW_BY_POINTS, IB_HOW_BY_EXTREMES, IB_HOW_UNBOUNDED = 0, 1, 2, 3, 4, 5
IB_ALL_EXTREMES = 1


def _implicit_one(A, l, u, tol, flags, o):
    """One polyhedron by the method of qpn_implicit_bounds (A [r, d] math layout).
    -> (status, fail_row, eq [r] uint8, vals [r], how [r] int32, lo [r], hi [r], lps, iters)."""
    r, d = A.shape
    every = bool(flags & IB_ALL_EXTREMES)
    eq = np.zeros(r, np.uint8); vals = np.full(r, INF); how = np.full(r, IB_HOW_UNDECIDED, np.int32)
    lo = np.full(r, np.nan); hi = np.full(r, np.nan)
    with np.errstate(all="ignore"):
        # (0) explicit rows
        explicit = (np.abs(l - u) <= tol) | (l == u)
        eq[explicit] = 1; vals[explicit] = 0.5 * (l[explicit] + u[explicit]); how[explicit] = IB_HOW_EXPLICIT
        if np.any(~explicit & (l > u)):                     # crossed bounds: no LP is started
            return IB_EMPTY, -1, eq, vals, how, lo, hi, 0, 0
        # (a) the feasibility solve: steps 1-8 with c = 0
        status, S, x = _lp_feasible(A, l, u, o)
        lps, iters = 1, S.iters
        if status != LP_OPTIMAL:
            return {LP_INFEASIBLE: IB_EMPTY, LP_ITER_LIMIT: IB_ITER_LIMIT}.get(status, IB_FAILURE), -1, eq, vals, how, lo, hi, lps, iters

        def rows_at(x):                                     # A x on the unscaled rows, columns ascending
            s = np.zeros(r)
            for j in range(d):
                s = s + A[:, j] * x[j]
            return s

        # (b) the witnesses
        s = rows_at(x)
        wlo, whi = s.copy(), s.copy()
        # (c) the rows from the last
        for i in range(r - 1, -1, -1):
            if explicit[i]:
                continue
            if not every and whi[i] - wlo[i] > tol:
                how[i] = IB_HOW_BY_POINTS
                continue
            decided = False
            for side in (0, 1):
                c = A[i].copy() if side == 0 else -A[i]
                lps += 1
                status, x, obj = _lp_resolve(S, c)          # (the cost row of c in the current dictionary as in §5g (e))
                iters += S.iters
                if status == LP_ITER_LIMIT:
                    return IB_ITER_LIMIT, i, eq, vals, how, lo, hi, lps, iters
                if status == LP_FAILURE:
                    return IB_FAILURE, i, eq, vals, how, lo, hi, lps, iters
                s = rows_at(x)
                wlo = np.where(s < wlo, s, wlo); whi = np.where(s > whi, s, whi)
                if side == 0:
                    lo[i] = -INF if status == LP_UNBOUNDED else obj
                    if not every:
                        if status == LP_UNBOUNDED:
                            how[i] = IB_HOW_UNBOUNDED; decided = True
                            break
                        if whi[i] - lo[i] > tol:
                            how[i] = IB_HOW_BY_POINTS; decided = True
                            break
                else:
                    hi[i] = INF if status == LP_UNBOUNDED else -obj
            if decided:
                continue
            if abs(lo[i]) < INF and abs(hi[i]) < INF and abs(lo[i] - hi[i]) <= tol:
                eq[i] = 1; vals[i] = 0.5 * (hi[i] + lo[i]); how[i] = IB_HOW_IMPLICIT
            else:
                how[i] = IB_HOW_BY_EXTREMES if abs(lo[i]) < INF and abs(hi[i]) < INF else IB_HOW_UNBOUNDED
    return IB_OK, -1, eq, vals, how, lo, hi, lps, iters


def implicit_bounds_host(Ac, l, u, tol=1e-4, all_extremes=False, opts=None):
    """The numpy twin of Engine.implicit_bounds (qpn_implicit_bounds), the normative statement of the method; every output of
    the kernel is bit-equal to it.  `implicit_bounds` (src/sets.jl:660-713) with one job per polyhedron: Ac [polys, d, r] (ABI
    layout), l, u [polys, r] (+-inf allowed).

    (0) A row with |l - u| <= tol or l == u is EXPLICIT: eq = 1, val = 0.5 (l + u); no LP takes it as objective.  Another row
    with l > u makes the polyhedron EMPTY before any LP (lps = 0: the simplex keeps a nonbasic row at one of its bounds and would
    not see that they cross).  (a) solve_lps_host's steps 1-8 with c = 0 (the crash and phase 1, once; _lp_feasible): an infeasible all-zero row, or an INFEASIBLE end whose
    Farkas certificate holds, is EMPTY, a certificate that fails FAILURE, ITER_LIMIT itself; the polyhedron stops there, its other
    rows keep eq = 0, val = +inf, UNDECIDED.  (b) witnesses: s = A x at the end point on the unscaled rows, columns ascending
    (acc = acc + a * x); wlo = whi = s, and after every later solve whose certificate holds wlo = s where s < wlo, whi = s where
    s > whi.  (c) the rows r - 1 ... 0 that are not explicit: whi - wlo > tol is BY_POINTS without an LP; otherwise the minimum, c =
    +a_i from the current basis (the cost row as in issubset_pairs_host (e), fresh step and degeneracy counters, the loop, the
    point and step 9's check: _lp_resolve): a certified ray gives lo = -inf, UNBOUNDED; an optimum lo = obj, and whi - lo > tol is BY_POINTS;
    then the maximum with c = -a_i: hi = -obj or +inf.  eq = lo, hi finite and |lo - hi| <= tol: val = 0.5 (hi + lo), IMPLICIT;
    else BY_EXTREMES, or UNBOUNDED when one of the two is infinite.  ITER_LIMIT, or an INFEASIBLE end or a failed certificate that
    the rebuild and the second loop of _lp_finish do not mend, in one of these solves ends the polyhedron with that status and
    fail_row = i.  all_extremes (QPN_IB_ALL_EXTREMES): no BY_POINTS and
    no early exit after an unbounded minimum; every row that is not explicit gets both extremes and is decided by them alone.
    -> dict(status [polys] int32 (IB_*), fail_row [polys] int32 (-1 without), eq [polys, r] uint8, vals [polys, r] (+inf where eq
    = 0), how [polys, r] int32 (IB_HOW_*), lo, hi [polys, r] (NaN where no LP computed them), lps [polys] int32 (solves started,
    the feasibility solve counted), iters [polys] int32 (all steps))."""
    Ac = np.asarray(Ac, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    polys, d, r = Ac.shape
    o = dict(LP_DEFAULT_OPTS)
    o.update(opts or {})
    flags = IB_ALL_EXTREMES if all_extremes else 0
    out = dict(status=np.zeros(polys, np.int32), fail_row=np.full(polys, -1, np.int32), eq=np.zeros((polys, r), np.uint8),
               vals=np.full((polys, r), INF), how=np.zeros((polys, r), np.int32), lo=np.full((polys, r), np.nan),
               hi=np.full((polys, r), np.nan), lps=np.zeros(polys, np.int32), iters=np.zeros(polys, np.int32))
    for b in range(polys):
        got = _implicit_one(np.ascontiguousarray(Ac[b].T), l[b], u[b], float(tol), flags, o)
        for k, v in zip(("status", "fail_row", "eq", "vals", "how", "lo", "hi", "lps", "iters"), got):
            out[k][b] = v
    return out


# ---- irredundant bounds (qpn_irredundant_bounds): one job per polyhedron, the numpy twin -----------------------------------------
RED_UNDECIDED, RED_NONE, RED_KEPT_EQUALITY, RED_REMOVED_ZERO_ROW, RED_KEPT_UNBOUNDED, RED_KEPT_BY_OPTIMUM, RED_REMOVED = 0, 1, 2, 3, 4, 5, 6


def _red_relax(S, lw, uw, i, side):
    """Bound `side` (0 lower, 1 upper) of row i leaves the working bounds: the unscaled copy the check reads (lw, uw = S.l, S.u)
    and the scaled one the loop reads.  Nothing else of the state changes: a nonbasic s_i keeps its value, now strictly inside."""
    if side == 0:
        lw[i] = -INF; S.ls[i] = -INF
    else:
        uw[i] = INF; S.us[i] = INF


def _red_restore(S, lw, uw, i, side, bound):
    """... and comes back: the unscaled value and bound * sc[i], the product the set-up made.  A basic s_i outside the bound is the
    next loop's phase-1 violation.  A nonbasic s_i whose value lies outside the restored bound takes the bound's value (the loop
    moves a nonbasic variable between its bounds and never towards them from outside)."""
    with np.errstate(all="ignore"):
        v = bound * S.sc[i]
    if side == 0:
        lw[i] = bound; S.ls[i] = v
    else:
        uw[i] = bound; S.us[i] = v
    for j in range(S.d):
        if S.cn[j] == S.d + i and (S.xn[j] < v if side == 0 else S.xn[j] > v):
            S.xn[j] = v


def _irredundant_one(A, l, u, tol, o):
    """One polyhedron by the method of qpn_irredundant_bounds (A [r, d] math layout).
    -> (status, fail_row, lr [r], ur [r], how [r, 2] int32, ext [r, 2], lps, iters)."""
    r, d = A.shape
    lw, uw = l.copy(), u.copy()                             # the working bounds; what an OK end returns
    how = np.full((r, 2), RED_UNDECIDED, np.int32); ext = np.full((r, 2), np.nan)

    def ended(status, row, lps, iters):                     # (e) the input back; a removal is no verdict any more
        how[(how == RED_REMOVED) | (how == RED_REMOVED_ZERO_ROW)] = RED_UNDECIDED
        return status, row, l.copy(), u.copy(), how, ext, lps, iters

    with np.errstate(all="ignore"):
        if np.any(l > u):                                   # crossed bounds: no LP is started
            return ended(IB_EMPTY, -1, 0, 0)
        # (a) the feasibility solve
        status, S, x = _lp_feasible(A, lw, uw, o)
        lps, iters = 1, S.iters
        if status != LP_OPTIMAL:
            return ended({LP_INFEASIBLE: IB_EMPTY, LP_ITER_LIMIT: IB_ITER_LIMIT}.get(status, IB_FAILURE), -1, lps, iters)
        # (b) the rows from the last, the lower bound before the upper
        for i in range(r - 1, -1, -1):
            if l[i] == u[i]:
                how[i] = RED_KEPT_EQUALITY
                continue
            if S.amax[i] == 0.0:                            # (a) has shown 0 within its bounds
                how[i] = RED_REMOVED_ZERO_ROW
                _red_relax(S, lw, uw, i, 0); _red_relax(S, lw, uw, i, 1)
                continue
            for side in (0, 1):
                bound = l[i] if side == 0 else u[i]
                if not abs(bound) < INF:
                    how[i, side] = RED_NONE
                    continue
                _red_relax(S, lw, uw, i, side)
                c = A[i].copy() if side == 0 else -A[i]
                lps += 1
                status, x, obj = _lp_resolve(S, c)
                iters += S.iters
                if status == LP_ITER_LIMIT:
                    return ended(IB_ITER_LIMIT, i, lps, iters)
                if status == LP_FAILURE:
                    return ended(IB_FAILURE, i, lps, iters)
                # (c) the verdict
                margin = tol * max(1.0, abs(bound))
                if status == LP_UNBOUNDED:
                    ext[i, side] = -INF if side == 0 else INF
                    how[i, side] = RED_KEPT_UNBOUNDED
                else:
                    e = obj if side == 0 else -obj
                    ext[i, side] = e
                    beyond = e < bound - margin if side == 0 else e > bound + margin
                    how[i, side] = RED_KEPT_BY_OPTIMUM if beyond else RED_REMOVED
                if how[i, side] != RED_REMOVED:
                    _red_restore(S, lw, uw, i, side, bound)     # (d)
    return IB_OK, -1, lw, uw, how, ext, lps, iters


def irredundant_bounds_host(Ac, l, u, tol=1e-8, opts=None):
    """The numpy twin of Engine.irredundant_bounds (qpn_irredundant_bounds), the normative statement of the method; every output of
    the kernel is bit-equal to it.  Which bounds of {x : l <= A x <= u} the other bounds imply, one job per polyhedron: Ac [polys, d, r]
    (ABI layout), l, u [polys, r] (+-inf allowed).  The reference gets irredundant pieces from `project` (src/sets.jl:501-523: vertices,
    then facets); this engine projects by elimination and prunes afterwards.

    A bound implied by the others is found only with that bound out of the way: a sum of two facet rows is tight exactly where both
    are, so its extreme over the whole set equals its bound.  The method therefore relaxes the bound it tests, and a removed bound
    stays removed for every later test, which keeps one of two equal rows.

    A row with l > u makes the polyhedron EMPTY before any LP (lps = 0), as in implicit_bounds_host (0).  (a) _lp_feasible once
    over working copies of l and u: an infeasible all-zero row, or an INFEASIBLE end whose Farkas certificate holds, is EMPTY, a
    certificate that fails FAILURE, ITER_LIMIT itself (the codes are IB_*).  (b) the rows r - 1 ... 0 (generated Fourier-Motzkin rows
    come last and go first), on each the lower bound before the upper: l == u is KEPT_EQUALITY on both sides, no LP; an all-zero row
    (max|a_i| = 0) has both bounds REMOVED_ZERO_ROW, no LP; an infinite bound is NONE; any other bound is relaxed to -+inf in the
    working bounds, unscaled (what step 9's check reads) and scaled (what the loop reads), nothing else of the state changing, and
    _lp_resolve runs c = +a_i (lower) or c = -a_i (upper) from the basis the previous solve left.  (c) a certified ray: KEPT_UNBOUNDED,
    ext = -+inf; an optimum, ext = obj (lower) or -obj (upper): ext < l - tol max(1, |l|) (ext > u + tol max(1, |u|)) is
    KEPT_BY_OPTIMUM, anything else REMOVED and the bound stays infinite.  ITER_LIMIT or FAILURE of the solve ends the polyhedron
    with fail_row = i.  (d) a kept bound is restored: the unscaled value and bound * sc_i.  A basic s_i now outside it is a phase-1
    violation the next solve's loop repairs (the phase is decided before every step).  A nonbasic s_i whose value lies outside the
    restored bound takes the bound's value.  (The loop does not produce that state: a nonbasic value is where the set-up put it, or
    a bound the variable reached, and the relaxed side has none to reach; the rule is there so that the state after a restore is
    one the loop is defined on whatever the solve did, and tests/test_irredundant_host.py exercises it on a state made by hand.)
    (e) a polyhedron that does not end OK returns lr = l, ur = u, and a REMOVED / REMOVED_ZERO_ROW becomes UNDECIDED again: the
    caller gets a finished pruning or its input back.  The other verdicts, and ext, stay as they were reached.
    -> dict(status [polys] int32 (IB_*), fail_row [polys] int32 (-1 without), lr, ur [polys, r] (the input, a removed bound -+inf),
    how [polys, r, 2] int32 (RED_*, [.., 0] the lower bound), ext [polys, r, 2] (the extreme an LP found, NaN where none ran),
    lps [polys] int32 (solves started, the feasibility solve counted), iters [polys] int32 (all steps))."""
    Ac = np.asarray(Ac, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    polys, d, r = Ac.shape
    o = dict(LP_DEFAULT_OPTS)
    o.update(opts or {})
    out = dict(status=np.zeros(polys, np.int32), fail_row=np.full(polys, -1, np.int32), lr=np.zeros((polys, r)), ur=np.zeros((polys, r)),
               how=np.zeros((polys, r, 2), np.int32), ext=np.full((polys, r, 2), np.nan), lps=np.zeros(polys, np.int32),
               iters=np.zeros(polys, np.int32))
    for b in range(polys):
        got = _irredundant_one(np.ascontiguousarray(Ac[b].T), l[b], u[b], float(tol), o)
        for k, v in zip(("status", "fail_row", "lr", "ur", "how", "ext", "lps", "iters"), got):
            out[k][b] = v
    return out


# ---- emptiness with open bounds (qpn_exemplar_polys): one job per polyhedron, the numpy twin -------------------------------------
EX_MEMBER,EX_MEMBER_BAND, EX_EMPTY_SLACK, EX_EMPTY_OPEN, EX_ITER_LIMIT, EX_FAILURE, EX_NOT_NEAR = 0, 1, 2, 3, 4, 5, 6
EX_MAX_N, EX_MAX_D, PROD_MAX_K = 511, 255, 32


def exemplar_rows(A, l, u, slack_cap=1.0):
    """The slack LP of `exemplar` (src/sets.jl:608-619) over {x : l <= A x <= u} (A [n, d] math layout) in the variables (x, eps):
    rows i < n: [a_i, 1] >= l_i; rows n + i: [-a_i, 1] >= -u_i; row 2 n: eps >= -slack_cap.  -> (A2 [2 n + 1, d + 1], l2, u2 = +inf).
    Leading axes are a batch of polyhedra of one shape: A [k, n, d], l, u [k, n] -> (A2 [k, 2 n + 1, d + 1], l2, u2 [k, 2 n + 1])."""
    lead, (n, d) = A.shape[:-2], A.shape[-2:]
    A2 = np.zeros(lead + (2 * n + 1, d + 1)); l2 = np.empty(lead + (2 * n + 1,))
    A2[..., :n, :d] = A; A2[..., n:2 * n, :d] = -A; A2[..., d] = 1.0
    l2[..., :n] = l; l2[..., n:2 * n] = -u; l2[..., 2 * n] = -slack_cap
    return A2, l2, np.full(lead + (2 * n + 1,), INF)


def _exemplar_one(A, l, u, open_lo, open_hi, tol, slack_cap, o):
    """One polyhedron by the method of qpn_exemplar_polys (A [n, d] math layout, open_lo / open_hi [n] bool).
    -> (empty, how, eps, x [d], row, lam [2 n + 1], iters)."""
    n, d = A.shape
    with np.errstate(all="ignore"):
        A2, l2, u2 = exemplar_rows(A, l, u, slack_cap)                      # (a)
        status, x, _, lam, _, iters = _lp_one(A2, l2, u2, 1.0 * A2[2 * n], o)
        if status != LP_OPTIMAL:                                            # (c)
            how = EX_ITER_LIMIT if status == LP_ITER_LIMIT else EX_FAILURE
            return 0, how, np.nan, np.zeros(d), -1, np.zeros(2 * n + 1), iters
        eps = x[d]                                                          # (b)
        row = -1
        if eps > tol:
            how = EX_EMPTY_SLACK
        elif eps > -tol:
            act_lo = (np.abs(lam[:n]) > tol) & open_lo & (np.abs(l) < INF)
            act_hi = (np.abs(lam[n:2 * n]) > tol) & open_hi & (np.abs(u) < INF)
            ids = np.concatenate([2 * np.nonzero(act_lo)[0], 2 * np.nonzero(act_hi)[0] + 1])
            how = EX_EMPTY_OPEN if ids.size else EX_MEMBER_BAND
            if ids.size:
                row = int(ids.min())
        else:
            how = EX_MEMBER
    empty = how in (EX_EMPTY_SLACK, EX_EMPTY_OPEN)
    return int(empty), how, eps, (np.zeros(d) if empty else x[:d]), row, lam, iters


def exemplar_polys_host(Ac, l, u, open_lo=None, open_hi=None, tol=1e-2, slack_cap=1.0, opts=None):
    """The numpy twin of Engine.exemplar_polys (qpn_exemplar_polys), the normative statement of the method; every output of the
    kernel is bit-equal to it.  `exemplar` / `isempty` (src/sets.jl:591-655) with one job per polyhedron: Ac [polys, d, n] (ABI
    layout), l, u [polys, n] (+-inf allowed), open_lo, open_hi [polys, n] (nonzero: that bound is open; None: closed).

    (a) The slack LP in (x, eps) (exemplar_rows): min eps over [a_i, 1] >= l_i, [-a_i, 1] >= -u_i, eps >= -slack_cap, the objective
    being the last row; solved as solve_lps_host solves a job (_lp_one: the data screen, the crash, the loop, step 9's check and
    at most one rebuild).  (b) On the certified optimum, eps = x[d]: eps > tol is EX_EMPTY_SLACK; eps > -tol is the band, where a
    bound is active when it is open, finite (an open flag on an infinite bound is ignored, src/sets.jl:354-356) and |lam_i| > tol
    (the lower bound of row i) or |lam_{n+i}| > tol (the upper): any active bound is EX_EMPTY_OPEN with row = the lowest 2 i +
    side, none EX_MEMBER_BAND; eps <= -tol is EX_MEMBER.  (c) LP_ITER_LIMIT is EX_ITER_LIMIT, every other end that is no certified
    optimum EX_FAILURE (the data screen included; the slack LP is feasible and bounded below, so INFEASIBLE and UNBOUNDED cannot be
    true answers): empty = 0, eps = NaN, x = 0, row = -1, lam = 0; iters is the count of the steps taken.
    -> dict(empty [polys] uint8, how [polys] int32 (EX_*), eps [polys], x [polys, d] (a member; zeros when empty or unanswered),
    row [polys] int32, lam [polys, 2 n + 1], iters [polys] int32)."""
    Ac = np.asarray(Ac, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    polys, d, n = Ac.shape
    flags = [np.zeros((polys, n), bool) if f is None else np.asarray(f).reshape(polys, n) != 0 for f in (open_lo, open_hi)]
    o = dict(LP_DEFAULT_OPTS)
    o.update(opts or {})
    out = dict(empty=np.zeros(polys, np.uint8), how=np.zeros(polys, np.int32), eps=np.zeros(polys), x=np.zeros((polys, d)),
               row=np.full(polys, -1, np.int32), lam=np.zeros((polys, 2 * n + 1)), iters=np.zeros(polys, np.int32))
    for b in range(polys):
        got = _exemplar_one(np.ascontiguousarray(Ac[b].T), l[b], u[b], flags[0][b], flags[1][b], float(tol), float(slack_cap), o)
        for k, v in zip(("empty", "how", "eps", "x", "row", "lam", "iters"), got):
            out[k][b] = v
    return out


# ---- emptiness of products of pieces (qpn_exemplar_products): one job per product, the numpy twin ------------------------------------
def exemplar_products_host(A, l, u, open_lo, open_hi, piece_row, factors, n, point=None, point_of=None, point_tol=1e-6, tol=1e-2,
                           slack_cap=1.0, opts=None, device=False):
    """The numpy twin of Engine.exemplar_products (qpn_exemplar_products), the normative statement of the method; every output of the
    kernel is bit-equal to it.  The emptiness test of the intersection tree (src/intersection.jl:66-105) with one job per product of
    pieces: the pool A [rows, d] (one ROW per pool row), l, u [rows] (+-inf allowed), open_lo, open_hi [rows] (nonzero: open; None:
    closed); piece p = the pool rows piece_row[p] .. piece_row[p + 1] - 1; factors [products, k] int32, -1 = no factor in that slot:
    product t is the intersection of its factors in slot order, its rows the factors' rows one after the other, n in all.  point
    [points, d], point_of [products] (both None: no closure test).

    (a) The map product row i -> pool row.  (b) The closure test at point[point_of[t]]: per row s_i = a_i'p over the ascending
    columns, acc = acc + a * p; near when l_i - point_tol <= s_i and s_i - point_tol <= u_i on every row, closed relations whatever
    the flags (`closure`, :74).  Not near: near = 0, how = EX_NOT_NEAR, empty = 0, eps = NaN, x = 0, lam = 0, iters = 0, row = the
    lowest 2 i + side violated; no LP.  (c) Otherwise near = 1 and _exemplar_one on the n gathered rows and flags: the outputs and
    codes of exemplar_polys_host; row counts product rows.  (d) A bad product -- a factor outside [-1, pieces), piece_row entries of a
    factor not 0 <= first <= last <= rows, rows that do not add up to n, a point_of outside [0, points) -- raises ValueError as host
    arrays do; device=True: it answers what the kernel answers for device arrays, near = 0, empty = 0, EX_FAILURE, eps = NaN, row =
    -1, zeros elsewhere.
    -> dict(near, empty [products] uint8, how [products] int32, eps [products], x [products, d], row [products] int32,
    lam [products, 2 n + 1], iters [products] int32)."""
    A = np.asarray(A, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    rows, d = A.shape
    piece_row = np.asarray(piece_row, dtype=np.int64); factors = np.asarray(factors, dtype=np.int64)
    pieces = len(piece_row) - 1
    products, k = factors.shape
    n = int(n)
    flags = [np.zeros(rows, bool) if f is None else np.asarray(f).reshape(rows) != 0 for f in (open_lo, open_hi)]
    if (point is None) != (point_of is None):
        raise ValueError("exemplar_products: point and point_of go together")
    if point is not None:
        point = np.asarray(point, dtype=np.float64).reshape(-1, d); point_of = np.asarray(point_of, dtype=np.int64)
    o = dict(LP_DEFAULT_OPTS)
    o.update(opts or {})
    out = dict(near=np.zeros(products, np.uint8), empty=np.zeros(products, np.uint8), how=np.full(products, EX_FAILURE, np.int32),
               eps=np.full(products, np.nan), x=np.zeros((products, d)), row=np.full(products, -1, np.int32),
               lam=np.zeros((products, 2 * n + 1)), iters=np.zeros(products, np.int32))
    for t in range(products):
        fs = [int(f) for f in factors[t] if f != -1]
        bad = None
        if any(f < -1 or f >= pieces for f in fs):
            bad = "factor out of range"
        elif any(not 0 <= piece_row[f] <= piece_row[f + 1] <= rows for f in fs):
            bad = "piece_row not ascending within the pool"
        elif sum(int(piece_row[f + 1] - piece_row[f]) for f in fs) != n:
            bad = "rows do not add up to n"
        elif point is not None and not 0 <= point_of[t] < len(point):
            bad = "point_of out of range"
        if bad:                                                             # (d)
            if not device:
                raise ValueError(f"exemplar_products: product {t}: {bad}")
            continue
        idx = np.concatenate([np.arange(piece_row[f], piece_row[f + 1]) for f in fs]).astype(np.int64)      # (a)
        low = -1
        if point is not None:                                               # (b)
            pt = point[point_of[t]]
            with np.errstate(all="ignore"):
                acc = np.zeros(n)
                for c in range(d):
                    acc = acc + A[idx, c] * pt[c]
                side = np.where(~(l[idx] - point_tol <= acc), 0, np.where(~(acc - point_tol <= u[idx]), 1, -1))
            hit = np.nonzero(side >= 0)[0]
            if hit.size:
                low = 2 * int(hit[0]) + int(side[hit[0]])
        if low >= 0:
            out["how"][t] = EX_NOT_NEAR; out["row"][t] = low
            continue
        out["near"][t] = 1                                                  # (c)
        got = _exemplar_one(np.ascontiguousarray(A[idx]), l[idx], u[idx], flags[0][idx], flags[1][idx], float(tol), float(slack_cap), o)
        for key, v in zip(("empty", "how", "eps", "x", "row", "lam", "iters"), got):
            out[key][t] = v
    return out


# ---- the intersection tree of combine (qpn_intersection_trees): prefixes pruned depth by depth, the numpy twin -------------------------
TREE_MAX_L, TREE_MAX_CAP = 32, 1 << 22


def intersection_trees_host(A, l, u, open_lo, open_hi, piece_row, L, list_ptr, list_mem, list_red, cap, point=None, point_of=None,
                            point_tol=1e-6, tol=1e-2, slack_cap=1.0, opts=None, device=False):
    """The numpy twin of Engine.intersection_trees (qpn_intersection_trees), the normative statement of the method; every output
    of the entry is equal to it.  The lazy enumeration of `combine` (src/qp_processing.jl:260-291; IntersectionRoot's walk,
    src/intersection.jl:66-105, :116-138), breadth first: `trees` trees of one depth L over the pool of exemplar_products_host (A
    [rows, d] one ROW per pool row, l, u, open_lo, open_hi [rows], piece_row [pieces + 1]).  list_ptr [trees L + 1] and list_mem
    form a CSR: list g L + t holds the pieces of union t of tree g, in the reference's order, its last list_red[g L + t] members
    being complement pieces (the redzone, :123).  point [points, d], point_of [trees] (both None: no closure test).  cap: the most
    tuples a frontier or a depth's candidates may hold.

    (0) Near: a member of a list stays when every row of its piece passes the closure test of exemplar_products_host (b) at the
    tree's point (acc = acc + a * p over the ascending columns, closed relations whatever the flags); the order of the rest is
    kept.  No point: every member is near.  (1) Expand: F_0 is one empty tuple per tree; for t = 1 .. L the candidates are, for
    every tuple of F_(t-1) in order and every near member of list t in order, the tuple with that member appended -- at t = L a
    candidate whose members are all complement pieces is not formed.  A candidate is one job of exemplar_products_host: its tuple
    as factors, -1 from slot t on, n = its rows, no point.  It is kept when empty == 0: EX_ITER_LIMIT and EX_FAILURE are no
    answer, the candidate stays and is counted in unanswered[t - 1].  F_t = the kept candidates in candidate order; tested[t - 1]
    and alive[t - 1] are the two counts.  (2) The leaves are F_L in order: by tree, then lexicographic in list positions.
    (3) A depth that forms more than cap candidates ends the call: overflow = that depth (1-based), tested of that depth = the
    count it formed, no count after it, no leaves, tree_leaves 0.  (4) list_ptr ascends as a whole, 0 <= list_ptr[i] <=
    list_ptr[i + 1] <= len(list_mem) -- lists must not overlap in list_mem --: where it does not, every tree of the call is bad.  A
    tree is bad when a list_red is outside [0, its list's length], a member is outside [0, pieces), a member's piece_row entries
    are not 0 <= first < last <= rows (a piece of no rows included), the longest pieces of its lists add up to more than EX_MAX_N
    rows, or its point_of is outside [0, points): ValueError as host arrays do; device=True: the tree forms no candidate and
    answers tree_leaves = -1, as the entry does for device arrays.
    -> dict(leaves [n_leaves, L] int32 (pool pieces), leaf_tree [n_leaves] int32, leaf_how [n_leaves] int32 (EX_*), n_leaves int,
    tree_leaves [trees] int32, tested, alive, unanswered [L] int64, overflow int)."""
    A = np.asarray(A, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    rows, d = A.shape
    piece_row = np.asarray(piece_row, dtype=np.int64)
    list_ptr = np.asarray(list_ptr, dtype=np.int64); list_mem = np.asarray(list_mem, dtype=np.int64).reshape(-1)
    list_red = np.asarray(list_red, dtype=np.int64)
    pieces, L, cap, M = len(piece_row) - 1, int(L), int(cap), len(list_mem)
    trees = len(list_red) // L if L > 0 else 0
    if not 2 <= L <= TREE_MAX_L or not 1 <= cap <= TREE_MAX_CAP or not 1 <= d <= EX_MAX_D:
        raise ValueError("intersection_trees: 2 <= L <= 32, 1 <= cap <= 2^22, 1 <= d <= 255")
    if len(list_red) != trees * L or len(list_ptr) != trees * L + 1 or (point is None) != (point_of is None):
        raise ValueError("intersection_trees: inconsistent arguments")
    if point is not None:
        point = np.asarray(point, dtype=np.float64).reshape(-1, d); point_of = np.asarray(point_of, dtype=np.int64)
    out = dict(leaves=np.zeros((0, L), np.int32), leaf_tree=np.zeros(0, np.int32), leaf_how=np.zeros(0, np.int32), n_leaves=0,
               tree_leaves=np.zeros(trees, np.int32), tested=np.zeros(L, np.int64), alive=np.zeros(L, np.int64),
               unanswered=np.zeros(L, np.int64), overflow=0)
    size = lambda f: int(piece_row[f + 1] - piece_row[f])
    # (4) the lists must not overlap in list_mem: the offsets ascend as a whole, or no tree is walked
    csr_bad = bool(trees) and bool(np.any(list_ptr[:-1] < 0) or np.any(np.diff(list_ptr) < 0) or np.any(list_ptr[1:] > M))
    if csr_bad and not device:
        raise ValueError("intersection_trees: list_ptr not ascending within list_mem")
    # (4) the trees, (0) the near members of their lists: (piece, is a complement piece)
    lists = [[[] for _ in range(L)] for _ in range(trees)]
    for g in range(trees):
        bad, longest = "list_ptr not ascending within list_mem" if csr_bad else None, 0
        for t in range(L if not bad else 0):
            p0, p1 = int(list_ptr[g * L + t]), int(list_ptr[g * L + t + 1])
            if not 0 <= p0 <= p1 <= M:
                bad = "list_ptr not ascending within list_mem"
                break
            mem = [int(f) for f in list_mem[p0:p1]]
            if not 0 <= list_red[g * L + t] <= p1 - p0:
                bad = "list_red outside its list"
            elif any(not 0 <= f < pieces for f in mem):
                bad = "member out of range"
            elif any(not 0 <= piece_row[f] < piece_row[f + 1] <= rows for f in mem):
                bad = "a member's piece_row entries are not 0 <= first < last <= rows"
            if bad:
                break
            longest += max([size(f) for f in mem], default=0)
        if not bad and longest > EX_MAX_N:
            bad = "the longest pieces of the lists add up to more than 511 rows"
        if not bad and point is not None and not 0 <= point_of[g] < len(point):
            bad = "point_of out of range"
        if bad:
            if not device:
                raise ValueError(f"intersection_trees: tree {g}: {bad}")
            out["tree_leaves"][g] = -1
            continue
        for t in range(L):
            p0, p1 = int(list_ptr[g * L + t]), int(list_ptr[g * L + t + 1])
            for j in range(p0, p1):
                f = int(list_mem[j])
                if point is not None:
                    idx = np.arange(piece_row[f], piece_row[f + 1])
                    pt = point[point_of[g]]
                    with np.errstate(all="ignore"):
                        acc = np.zeros(len(idx))
                        for c in range(d):
                            acc = acc + A[idx, c] * pt[c]
                        if not (np.all(l[idx] - point_tol <= acc) and np.all(acc - point_tol <= u[idx])):
                            continue
                lists[g][t].append((f, j >= p1 - int(list_red[g * L + t])))
    # (1) breadth first: a tuple of the frontier is (tree, members, all of them complement pieces)
    frontier = [(g, (), True) for g in range(trees)]
    hows = []
    for t in range(1, L + 1):
        cands = []
        for g, tup, allc in frontier:
            for f, comp in lists[g][t - 1]:
                if t == L and allc and comp:
                    continue
                cands.append((g, tup + (f,), allc and comp))
        out["tested"][t - 1] = len(cands)
        if len(cands) > cap:                                                # (3)
            out["overflow"] = t
            return out
        ns = [sum(size(f) for f in c[1]) for c in cands]
        empty = np.zeros(len(cands), bool); how = np.zeros(len(cands), np.int32)
        for n in sorted(set(ns)):
            at = [i for i, v in enumerate(ns) if v == n]
            factors = np.full((len(at), L), -1, np.int64)
            for k, i in enumerate(at):
                factors[k, :t] = cands[i][1]
            got = exemplar_products_host(A, l, u, open_lo, open_hi, piece_row, factors, n, tol=tol, slack_cap=slack_cap, opts=opts)
            empty[at] = got["empty"] != 0; how[at] = got["how"]
        keep = np.nonzero(~empty)[0]
        frontier = [cands[i] for i in keep]
        hows = how[keep]
        out["alive"][t - 1] = len(keep)
        out["unanswered"][t - 1] = int(np.isin(hows, (EX_ITER_LIMIT, EX_FAILURE)).sum())
    n_leaves = len(frontier)                                                # (2)
    out["n_leaves"] = n_leaves
    out["leaves"] = np.array([c[1] for c in frontier], np.int32).reshape(n_leaves, L)
    out["leaf_tree"] = np.array([c[0] for c in frontier], np.int32)
    out["leaf_how"] = np.asarray(hows, np.int32).reshape(n_leaves)
    for g in out["leaf_tree"]:
        out["tree_leaves"][g] += 1
    return out


# ---- interior members (qpn_assemble_interior_nodes, qpn_members_outside): the numpy twins ------------------------------------------
def _interior_row_classes(l, u):
    """The row classes of interior members -> (eq, lo, hi) [B, r] bool: equality rows (finite l == u), other rows with a finite
    lower bound, other rows with a finite upper bound; and the slot counts (ne, nlo, nhi), the largest number of each of any item."""
    eq = np.isfinite(l) & (l == u)
    lo = ~eq & np.isfinite(l); hi = ~eq & np.isfinite(u)
    return (eq, lo, hi), (int(eq.sum(1).max(initial=0)), int(lo.sum(1).max(initial=0)), int(hi.sum(1).max(initial=0)))


def interior_member_counts(l, u):
    """The slot counts (ne, nlo, nhi) of a batch's interior-member records: the largest number of equality rows (finite l == u),
    of other rows with a finite lower bound and of other rows with a finite upper bound of any item.  l, u [B, r]."""
    return _interior_row_classes(np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64))[1]


def interior_member_records(A, l, u, delta):
    """The node records of the interior-member queries of B polyhedra of one size, A [B, r, d] (math layout), l, u [B, r], packed
    straight into the ABI's column-major blocks -> (Qc [B, nf, nf], qd [B, nf], Ac [B, nf, mp], ll, uu [B, mp]) with
    nf = d + 1 + ne, mp = max(16, nlo + nhi rounded up to 16), (ne, nlo, nhi) = interior_member_counts(l, u); p = 1, R = 0, B = 0.
    The counts of equality / lower / upper rows differ from piece to piece: the free block is padded with idle multipliers (a unit
    diagonal entry, no coupling: mu = 0) and the rows with inert ones (0'z in (-inf, inf)) up to the batch's largest.
    This is the numpy twin of Engine.assemble_interior_nodes (qpn_assemble_interior_nodes), and the route of engines without it."""
    A = np.asarray(A, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    B, r, d = A.shape
    (eq, lo, hi), (ne, nlo, nhi) = _interior_row_classes(l, u)

    def pick(mask, cnt):                                  # first `cnt` row indices with the mask set, ascending; valid flags
        order = np.argsort(~mask, axis=1, kind="stable")[:, :cnt]
        return order, np.take_along_axis(mask, order, axis=1)

    (E, Ev), (LO, LOv), (HI, HIv) = pick(eq, ne), pick(lo, nlo), pick(hi, nhi)
    bidx = np.arange(B)[:, None]
    rows_of = lambda sel, valid: A[bidx, sel] * valid[:, :, None]        # (whole rows by index pairs: no index broadcast over d)
    nf = d + 1 + ne                                       # free block: [x; eps; mu_E]
    mi = nlo + nhi
    mp = max(16, -(-mi // 16) * 16)
    Qc = np.zeros((B, nf, nf)); qd = np.zeros((B, nf)); Ac = np.zeros((B, nf, mp))
    ll = np.full((B, mp), -INF); uu = np.full((B, mp), INF)
    ar = np.arange(d + 1)
    Qc[:, ar, ar] = delta
    qd[:, d] = 1.0
    if ne:
        AE = rows_of(E, Ev)                               # [B, ne, d], zero rows in the idle slots
        # math layout: Qd' = [[delta I, -A_E'], [A_E, 0]] (eps column of A_E is 0); Qc is its transpose per item
        Qc[:, d + 1:, :d] = -AE
        Qc[:, :d, d + 1:] = np.swapaxes(AE, 1, 2)
        je = d + 1 + np.arange(ne)
        Qc[:, je, je] = np.where(Ev, 0.0, 1.0)            # idle multipliers: 1 * mu = 0
        qd[:, d + 1:] = np.where(Ev, -np.take_along_axis(l, E, axis=1), 0.0)
    if nlo:
        Ac[:, :d, :nlo] = np.swapaxes(rows_of(LO, LOv), 1, 2); Ac[:, d, :nlo] = np.where(LOv, 1.0, 0.0)
        ll[:, :nlo] = np.where(LOv, np.take_along_axis(l, LO, axis=1), -INF)
    if nhi:
        Ac[:, :d, nlo:mi] = np.swapaxes(rows_of(HI, HIv), 1, 2); Ac[:, d, nlo:mi] = np.where(HIv, -1.0, 0.0)
        uu[:, nlo:mi] = np.where(HIv, np.take_along_axis(u, HI, axis=1), INF)
    return Qc, qd, Ac, ll, uu


def members_outside_host(Ajc, lj, uj, X, pi, pj, t):
    """The numpy twin of Engine.members_outside (qpn_members_outside), same operations in the same order: out [pairs] uint8, 1 where
    member X[pi[q]] violates a row of piece pj[q] -- a.x < l - t or a.x > u + t -- with a.x summed over ascending columns,
    acc = acc + a * x[c].  Ajc [Bj, d, rj] (the pieces' matrices in the ABI layout), lj, uj [Bj, rj], X [Bi, d]."""
    Ajc = np.asarray(Ajc, dtype=np.float64); lj = np.asarray(lj, dtype=np.float64); uj = np.asarray(uj, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64); pi = np.asarray(pi, dtype=np.int64); pj = np.asarray(pj, dtype=np.int64)
    Bj, d, rj = Ajc.shape
    out = np.zeros(len(pi), np.uint8)
    step = max(1, (1 << 24) // max(1, rj))                # (pairs x rows doubles per slice)
    for s in range(0, len(pi), step):
        qi, qj = pi[s:s + step], pj[s:s + step]
        acc = np.zeros((len(qi), rj))
        for c in range(d):
            acc = acc + Ajc[qj, c, :] * X[qi, c][:, None]
        with np.errstate(invalid="ignore"):
            out[s:s + step] = np.any((acc < lj[qj] - t) | (acc > uj[qj] + t), axis=1)
    return out


def members_outside_lists_host(Ajc, lj, uj, X, ok, list_ptr, list_mem, list_of, self_pos, word_ptr, t, strict=False):
    """The numpy twin of Engine.members_outside_lists (qpn_members_outside_lists) and its normative statement: every member of a
    list against every piece of the same list, said by the lists.  One pack of second pieces Ajc [Bj, d, rj], lj, uj [Bj, rj];
    members X [Bi, d] with flags ok [Bi]; list_ptr [lists + 1] and list_mem form a CSR (position s of list a is row
    list_mem[list_ptr[a] + s] of X, -1 = no member); list_of, self_pos [Bj]: the list of piece j and its own position there;
    word_ptr [Bj + 1]: piece j owns the words [word_ptr[j], word_ptr[j + 1]) of bits, at least ceil(k / 32) for a list of k.
    -> (bits [word_ptr[Bj]] uint32, undecided [Bj] int32).  Bit (s & 31) of word (s >> 5) of piece j's segment is 1 when
    s != self_pos[j], the member at position s exists and is ok, and members_outside_host says it lies outside piece j -- the
    verdicts ARE members_outside_host's, on the enumerated pairs -- and every other bit of the segment is 0; undecided[j] counts
    the positions s != self_pos[j] of the list whose bit is 0.
    Bad items, strict=False (the entry's device mode): a piece whose list_of or self_pos is out of range, or whose segment is
    shorter than its list needs (or not inside bits at all: then nothing of it is written), has its whole segment 0 and
    undecided = max(k - 1, 0), or 0 when the list itself is bad (list_of out of range, or its list_ptr entries decreasing or
    outside list_mem); a list_mem entry outside [-1, Bi) answers 1 for its position, other than self_pos (the convention of
    qpn_members_outside: not settled here).  strict=True (host mode): any of these raises ValueError, as do list_ptr or
    word_ptr that do not start at 0 or decrease."""
    Ajc = np.asarray(Ajc, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64); ok = np.asarray(ok).astype(bool)
    list_ptr = np.asarray(list_ptr, dtype=np.int64); list_mem = np.asarray(list_mem, dtype=np.int64)
    list_of = np.asarray(list_of, dtype=np.int64); self_pos = np.asarray(self_pos, dtype=np.int64)
    word_ptr = np.asarray(word_ptr, dtype=np.int64)
    Bj, Bi, lists = Ajc.shape[0], X.shape[0], len(list_ptr) - 1
    M, W = int(list_ptr[-1]), int(word_ptr[-1]) if Bj else 0

    def bad(what):
        if strict:
            raise ValueError(f"members_outside_lists: {what}")

    if strict:
        if list_ptr[0] != 0 or word_ptr[0] != 0:
            bad("list_ptr and word_ptr start at 0")
        if np.any(np.diff(list_ptr) < 0) or np.any(np.diff(word_ptr) < 0):
            bad("list_ptr or word_ptr is not monotone")
        if np.any((list_mem[:M] < -1) | (list_mem[:M] >= Bi)):
            bad("list_mem entry out of range")
    bits = np.zeros(max(W, 0), np.uint32)
    undecided = np.zeros(Bj, np.int32)
    pi, pj, at = [], [], []                               # the enumerated pairs; (piece, positions) of each run of them
    kept = {}
    for j in range(Bj):
        w0, w1 = int(word_ptr[j]), int(word_ptr[j + 1])
        seg_ok = 0 <= w0 <= w1 <= W
        a, k = int(list_of[j]), -1
        if 0 <= a < lists:
            p0, p1 = int(list_ptr[a]), int(list_ptr[a + 1])
            if 0 <= p0 <= p1 <= M:
                k = p1 - p0
        elif lists:
            bad("list_of out of range")
        sp = int(self_pos[j])
        if lists and k >= 0 and not 0 <= sp < k:
            bad("self_pos out of range")
        if lists and k >= 0 and seg_ok and w1 - w0 < -(-k // 32):
            bad("segment of bits shorter than its list")
        if not seg_ok or k < 0 or not 0 <= sp < k or w1 - w0 < -(-k // 32):
            undecided[j] = max(k - 1, 0)
            continue
        mem = list_mem[p0:p1]
        pos = np.arange(k)
        inr = (mem >= 0) & (mem < Bi)
        use = inr & (pos != sp)
        use[use] = ok[mem[use]]
        kept[j] = (pos != sp) & ((mem < -1) | (mem >= Bi))
        pi.append(mem[use]); pj.append(np.full(int(use.sum()), j, np.int64)); at.append((j, pos[use]))
    out = members_outside_host(Ajc, lj, uj, X, np.concatenate(pi), np.concatenate(pj), t) if pi else np.zeros(0, np.uint8)
    q0 = 0
    for j, pos in at:
        k = len(kept[j])
        flag = kept[j].copy()
        flag[pos] = out[q0:q0 + len(pos)].astype(bool)
        q0 += len(pos)
        nwk = -(-k // 32)
        padded = np.zeros(32 * nwk, bool); padded[:k] = flag
        w0 = int(word_ptr[j])
        bits[w0:w0 + nwk] = np.packbits(padded, bitorder="little").view("<u4")
        undecided[j] = k - 1 - int(flag.sum())            # (the own position's bit is never set)
    return bits, undecided
