"""A plain numpy statement of the Stage B pivot loop (the bounded-variable Lemke method on the Schur dictionary, rules as in
csrc/qpn_avi_schur.hip), kept for ONE purpose: to say which branches of the loop a node of tests/stage_b_cases.py takes.  The
oracle and the kernels report `pivots`, which counts basis changes AND bound flips (an entering variable that reaches its own
opposite bound before any row blocks it: no basis change); this walk counts them apart and notes the direction of every flip.
It is no reference for values: tests/test_stage_b_cases_host.py accepts a walk only when its pivot count equals the oracle's.

pair k: p_k = (S lambda + c)_k in [l_k, u_k], d_k = lambda_k; ids p_k -> k, d_k -> m + k, artificial -> 2 m; column m is the
extra (covering) column."""
import numpy as np

INF = np.inf


def walk(Q, R, qd, A, B, l, u, w, piv_tol, feas_tol, max_pivots=0, slack=1e-10):
    """-> dict(status, pivots (Stage B only), basis_changes, flips: list of +1 (a variable went from lo to hi) / -1)."""
    m = l.shape[0]
    g = qd + R @ w
    S = A @ np.linalg.solve(Q, A.T)
    xb = B @ w - A @ np.linalg.solve(Q, g)
    T = S.copy()
    lo0, hi0 = l.astype(float).copy(), u.astype(float).copy()
    lo, hi = lo0.copy(), hi0.copy()
    cls = np.where((lo0 == -INF) & (hi0 == INF), 2, 0)
    rng = hi0 - lo0
    sat = np.zeros(m, int)
    VTH, XC = 2 * m, m
    rowvar = np.arange(m)
    colvar = np.concatenate([m + np.arange(m), [VTH]])
    nbval = np.zeros(m + 1)
    tcol = np.zeros(m)
    out = dict(status=4, pivots=0, basis_changes=0, flips=[])
    viol = np.where(xb < lo, lo - xb, np.where(xb > hi, xb - hi, 0.0))
    theta0 = viol.max()
    if theta0 <= feas_tol:
        out["status"] = 1
        return out
    for k in range(m):
        if xb[k] < lo[k]:
            tgt = lo[k] + (theta0 - (lo[k] - xb[k]))
            if hi[k] < INF:
                tgt = min(tgt, 0.5 * (lo[k] + hi[k]))
            tcol[k] = (tgt - xb[k]) / theta0; xb[k] = tgt
        elif xb[k] > hi[k]:
            tgt = hi[k] - (theta0 - (xb[k] - hi[k]))
            if lo[k] > -INF:
                tgt = max(tgt, 0.5 * (lo[k] + hi[k]))
            tcol[k] = (tgt - xb[k]) / theta0; xb[k] = tgt
    nbval[XC] = theta0
    self_lim, c, sneg, elo, ehi = theta0, XC, True, 0.0, INF
    limit = max_pivots if max_pivots > 0 else 50 * 2 * m + 100
    while True:
        if out["pivots"] >= limit:
            out["status"] = 3
            return out
        cm = tcol.copy() if c == XC else T[:, c].copy()
        gdir = -cm if sneg else cm
        with np.errstate(divide="ignore", invalid="ignore"):
            rc = 1.0 / gdir
            tb = np.where(np.signbit(gdir), lo, hi)
            cnd = (np.abs(gdir) > piv_tol) & (np.abs(tb) < INF)
            dd = np.where(cnd, (tb - xb) * rc, INF)
            d1 = np.where(cnd, dd + slack * np.abs(rc), INF)
        dmax = min(d1.min(), self_lim)
        if dmax == INF:
            out["status"] = 2
            return out
        bal = dd <= dmax
        if not bal.any():
            # the entering variable reaches its own opposite bound first: no basis change
            xb = xb + (-self_lim if sneg else self_lim) * cm
            ve = colvar[c]
            if ve == VTH:
                out["status"] = 1
                return out
            k = int(ve)
            au = 0 if sneg else 1
            out["flips"].append(+1 if au else -1)
            nbval[c] = hi0[k] if au else lo0[k]
            sat[k] = au
            out["pivots"] += 1
            hit = np.flatnonzero(colvar == m + k)
            if len(hit) == 0:
                return out
            c = int(hit[0]); sneg = au != 0; self_lim = INF
            elo, ehi = (-INF, 0.0) if au else (0.0, INF)
            continue
        if bal.sum() == 1:
            r = int(np.flatnonzero(bal)[0])
        else:
            ag = np.where(bal, np.abs(gdir), -1.0)
            ag[bal & (rowvar == VTH)] = INF
            r = int(np.flatnonzero(bal & (ag == ag.max()))[0])
        step = max(dd[r], 0.0)
        leave_val, rcr = tb[r], rc[r]
        inv = -rcr if sneg else rcr
        delta = -step if sneg else step
        vl = int(rowvar[r])
        enter_val = nbval[c] + delta
        row = T[r, :].copy(); px = tcol[r]
        if c == XC:
            px = -1.0
        else:
            row[c] = -1.0
        v = row * inv; vx = px * inv
        tc0 = np.zeros(m) if c == XC else tcol
        xbn = xb + delta * cm; tcn = tc0 - cm * vx
        xbn[r] = enter_val; tcn[r] = -vx
        xb, tcol = xbn, tcn
        T = T - np.outer(cm, v)
        if c != XC:
            T[:, c] = cm * inv
        T[r, :] = -v
        ve = int(colvar[c])
        rowvar[r] = ve; lo[r], hi[r] = elo, ehi
        colvar[c] = vl; nbval[c] = leave_val
        out["pivots"] += 1; out["basis_changes"] += 1
        if vl == VTH:
            out["status"] = 1
            return out
        k = vl if vl < m else vl - m
        if vl < m:
            au = 0 if np.signbit(rcr) else 1
            sat[k] = au; vn = m + k; sneg = au != 0; self_lim = INF
            elo, ehi = (0.0, 0.0) if cls[k] == 2 else ((-INF, 0.0) if au else (0.0, INF))
        else:
            au = sat[k]; vn = k; sneg = au != 0 and cls[k] != 2; self_lim = rng[k]
            elo, ehi = lo0[k], hi0[k]
        hit = np.flatnonzero(colvar == vn)
        if vn == ve or len(hit) == 0:
            return out
        c = int(hit[0])
