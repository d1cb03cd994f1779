"""Seeded node records that put verify_solution (src/qp_processing.jl:57-149) at the places where its kernels can go wrong.

Every case plants   q~ = A_bar lam* + r_perp   with lam* sign-feasible by a margin and r_perp exactly orthogonal to range(A_bar):
the active rows live on a random subset of the coordinates and r_perp on the others, so no rounding enters the orthogonality.
qd is then set so that Qd x + R w + qd is that q~.  Active rows sit at l (pos), u (neg) or l == u (both) up to a feasible
offset below 5e-4; inactive rows are at least 0.05 away from both bounds, so every class has a margin of ~1e-2.

make_case(...) -> dict(rec=(Qd, R, qd, Ad, B, l, u, xd, w), want="accept" | "reject", tag=...), math layout.
"""
from __future__ import annotations

import numpy as np

from verify_ref import xmatvec, two_prod

TOL = 1e-4
P = 2                                    # parameters per node


def _dyadic(rng, size, bits=8, lo=-1.0, hi=1.0):
    return np.round(rng.uniform(lo, hi, size) * 2 ** bits) / 2 ** bits


def _unit(v):
    return v / np.linalg.norm(v)


def _finish(rng, n, m, D, cls, lam, rperp, supp, qnorm=None, dense=True):
    """D (k x n) active rows, cls (k) in {1, 2, 3}, lam (k) multipliers of A_bar's columns (>= 0 on classes 1, 2);
    r_perp of norm rperp on the coordinates outside supp; qnorm rescales lam so that |A_bar lam| = qnorm."""
    k = D.shape[0]
    sg = np.where(cls == 2, -1.0, 1.0)
    Ab = (D * sg[:, None]).T
    g = Ab @ lam
    if qnorm is not None and np.linalg.norm(g) > 0:
        lam = lam * (qnorm / np.linalg.norm(g))
        g = Ab @ lam
    comp = np.setdiff1d(np.arange(n), supp)
    r = np.zeros(n)
    if rperp > 0:
        assert comp.size, "no room for r_perp"
        r[comp] = _unit(rng.standard_normal(comp.size)) * rperp
    qt = g + r
    x = _dyadic(rng, n)
    w = _dyadic(rng, P)
    Q = rng.standard_normal((n, n)) / n
    Q = Q + Q.T + 2 * np.eye(n)
    R = rng.standard_normal((n, P)) * 0.5
    qd = qt - Q @ x - R @ w
    A = rng.standard_normal((m, n)) / np.sqrt(n)
    Bm = rng.standard_normal((m, P)) * 0.3 if dense else np.zeros((m, P))
    rows = rng.permutation(m)[:k]
    A[rows] = D
    ax = xmatvec(A, x, extra=np.concatenate(two_prod(Bm, w[None, :]), axis=1))
    l = ax - rng.uniform(0.05, 1.0, m)
    u = ax + rng.uniform(0.05, 1.0, m)
    l[rng.random(m) < 0.2] = -np.inf
    u[rng.random(m) < 0.2] = np.inf
    off = rng.uniform(0.0, 5e-4, k)
    for t, (i, c) in enumerate(zip(rows, cls)):
        if c == 1:
            l[i] = ax[i] - off[t]; u[i] = np.inf if rng.random() < 0.5 else ax[i] + 1.0
        elif c == 2:
            u[i] = ax[i] + off[t]; l[i] = -np.inf if rng.random() < 0.5 else ax[i] - 1.0
        else:
            l[i] = u[i] = ax[i]
    return (Q, R, qd, A, Bm, l, u, x, w)


def _rows(rng, k, n, d):
    """k random unit rows supported on d random coordinates (returns rows, support)."""
    supp = np.sort(rng.permutation(n)[:d])
    D = np.zeros((k, n))
    D[:, supp] = rng.standard_normal((k, d))
    return D / np.linalg.norm(D, axis=1, keepdims=True), supp


def _classes(rng, k, p_free=0.15):
    c = rng.choice([1, 2], size=k)
    c[rng.random(k) < p_free] = 3
    return c


def _lams(rng, cls, lo=0.5, hi=2.0):
    lam = rng.uniform(lo, hi, cls.size)
    free = cls == 3
    lam[free] *= rng.choice([-1.0, 1.0], free.sum())
    return lam


def make_case(rng, n, m, k, family="generic", rperp=0.0, qnorm=1.0, theta=1e-3, pair="pp", tol=TOL):
    """One node with k active rows.  family: generic | parallel (pair pp / pn / eq, separation theta) | scale (row norms
    1e-3..1e3) | dup (an exact duplicate and a pos/neg copy of the same row) | signforce (one planted multiplier of the wrong
    sign: the bounded least squares decides)."""
    want = "accept" if rperp <= 0.3 * tol else "reject"
    extra = 0 if rperp == 0 and k < n else 1
    if family == "dup":
        kb = k - 2
        assert 2 <= kb <= n - extra
        D, supp = _rows(rng, kb, n, min(n - extra, kb + 2))
        cls = _classes(rng, kb)
        i = 0
        D = np.vstack([D, D[i], D[i + 1]])
        c1 = 1 if cls[i + 1] != 1 else 2
        cls = np.concatenate([cls, [cls[i]], [c1]])
        lam = _lams(rng, cls)
        lam[kb:] = 0.0                                  # the copies carry nothing; the duplicated rows' columns carry lam*
        if cls[i + 1] == 3:
            lam[i + 1] = abs(lam[i + 1])
        return dict(rec=_finish(rng, n, m, D, cls, lam, rperp, supp, qnorm), want=want, tag=f"dup k={k}")
    d = min(n - extra, k + max(2, k // 8))
    assert k <= d, "more active rows than the support can hold independently"
    D, supp = _rows(rng, k, n, d)
    cls = _classes(rng, k)
    lam = _lams(rng, cls)
    tag = f"{family} k={k}"
    if family == "parallel":
        a, b = 0, 1
        e = np.zeros(n); e[supp] = rng.standard_normal(supp.size)
        e = _unit(e - (e @ D[a]) * D[a])
        D[b] = _unit(D[a] + theta * e)
        lam[a], lam[b] = abs(lam[a]), abs(lam[b])
        if pair == "pp":
            cls[a] = cls[b] = 1
        elif pair == "pn":
            cls[a], cls[b] = 1, 2
            lam[a] = lam[b] = 1.0 / theta             # large positive multipliers: the pair's columns nearly cancel
        else:
            cls[a] = cls[b] = 3
        tag += f" {pair} theta={theta:.0e}"
    elif family == "scale":
        D = D * (10.0 ** rng.uniform(-3, 3, k))[:, None]
    elif family == "signforce":
        j = int(np.flatnonzero(cls != 3)[0]) if np.any(cls != 3) else 0
        cls[j] = 1
        lam[j] = -1.0                                 # r* ~ |lam_j| * dist(col_j, span(others)): a clear reject
        want = "reject"
    elif family != "generic":
        raise ValueError(family)
    return dict(rec=_finish(rng, n, m, D, cls, lam, rperp, supp, qnorm), want=want, tag=tag + f" |q|={qnorm:.0e} r={rperp:.0e}")


def exact_threshold_cases(rng, n=16, m=12):
    """One-hot rows of power-of-two scale, dyadic data, B = 0, Qd = I, R = 0: ax and q~ are exact in any summation order.
    Row 4's ax sits exactly at fl(l + 1e-2), fl(u - 1e-2), fl(l - 1e-3), fl(u + 1e-3) or one ulp inside / outside them, and q~
    has a component along row 4 that only an active row 4 explains: its class (and feasibility) decides flag and path, which
    every route must therefore reproduce bit for bit."""
    out = []
    spots = [("l+act", 0), ("l+act", -1), ("u-act", 0), ("u-act", +1), ("l-feas", 0), ("l-feas", -1),
             ("u+feas", 0), ("u+feas", +1)]
    for spot, ulp in spots:
        for rperp in (0.0, 30 * TOL):
            x = np.zeros(n)
            A = np.zeros((m, n))
            sc = np.ldexp(1.0, rng.integers(-3, 4, m))
            for i in range(m):
                A[i, i] = sc[i]
            l = np.full(m, -np.inf); u = np.full(m, np.inf)
            lam = np.zeros(m)
            # rows 0..3 active at their bound (pos, pos, neg, both) with dyadic x, the rest inactive; row 4 carries the spot
            xs = _dyadic(rng, m, bits=6)
            for i in range(m):
                x[i] = xs[i] / 1.0
            ax = sc * x[:m]
            l[0] = ax[0]; lam[0] = 0.75
            l[1] = ax[1] - 2.0 ** -12; lam[1] = 1.25
            u[2] = ax[2]; lam[2] = -0.5
            l[3] = u[3] = ax[3]; lam[3] = -0.375
            for i in range(5, m):
                l[i] = ax[i] - 0.5; u[i] = ax[i] + 0.5
            i = 4
            base = 0.25
            if spot == "l+act":
                l[i] = base; t = base + 1e-2; u[i] = np.inf
            elif spot == "u-act":
                u[i] = base; t = base - 1e-2; l[i] = -np.inf
            elif spot == "l-feas":
                l[i] = base; t = base - 1e-3; u[i] = np.inf
            else:
                u[i] = base; t = base + 1e-3; l[i] = -np.inf
            t = np.nextafter(t, np.inf) if ulp > 0 else (np.nextafter(t, -np.inf) if ulp < 0 else t)
            lam[i] = 0.5 if spot[0] == "l" else -0.5   # explained only if the row is active: its class decides the flag
            x[i] = t / sc[i]
            ax[i] = t
            qt = A.T @ lam                        # exact: one-hot rows, dyadic multipliers and scales
            if rperp:
                qt[m] = rperp                     # a coordinate no row touches
            Q = np.eye(n)
            R = np.zeros((n, P))
            qd = qt - x                           # Q x = x exactly
            w = _dyadic(rng, P)
            rec = (Q, R, qd, A, np.zeros((m, P)), l, u, x, w)
            out.append(dict(rec=rec, want=None, tag=f"exact {spot} ulp={ulp:+d} r={rperp:.0e}"))
    return out


def stack(cases):
    """Cases of one shape -> stacked arrays (Q, R, qd, A, B, l, u, xd, w[batch, p])."""
    return tuple(np.stack([c["rec"][j] for c in cases]) for j in range(9))


# ---- the route matrix of qpn_launch_verify_nodes (csrc/qpn_verify.hip) -------------------------------------------------------
# cell -> (n, m, active-row counts to draw from, batch); the 33..64 overflow cell is one batch of more than 256 nodes that all
# leave verify_node64 (k > 32): 256 of them find a slot of verify_wide_node's workspace, the rest go to verify_stage1<65>.
CELLS = {
    "node32":       (12, 16, (4, 9), None),
    "node32_full":  (32, 32, (10, 24), None),
    "node64":       (48, 48, (12, 30), None),
    "mid_slots":    (64, 64, (34, 56), None),
    "mid_overflow": (40, 40, (33, 36), 280),
    "wide_fast":    (96, 80, (40, 78), None),
    "wide_c5":      (256, 256, (70, 100), None),
    "wide_pivoted": (160, 140, (113, 128), None),
    "wide_stage":   (200, 160, (129, 150), None),
}
RPERP = (0.0, 0.3 * TOL, 3 * TOL, 30 * TOL)           # must accept, must accept, must reject, must reject


def route_of(n, m, k, cell):
    """The launcher's route for a node with k active rows (what the cell is meant to exercise is checked against it)."""
    if n > 64 or m > 64:
        return "wide_fast" if k <= 112 else ("wide_pivoted" if k <= 128 else "wide_stage")
    if n <= 32 and m <= 32:
        return "node32_full" if n == m == 32 else "node32"
    if k <= 32:
        return "node64"
    return "mid_overflow" if cell == "mid_overflow" else "mid_slots"


def cell_cases(cell, seed=7):
    """The cases of one cell: every family, every planted r_perp, every theta and pair type, every |q~|."""
    n, m, (k0, k1), batch = CELLS[cell]
    rng = np.random.default_rng([seed, sum(map(ord, cell))])
    ks = lambda: int(rng.integers(k0, k1 + 1))
    out = []
    for t, r in enumerate(RPERP):
        out.append(make_case(rng, n, m, ks(), "generic", rperp=r))
        out.append(make_case(rng, n, m, ks(), "scale", rperp=r))
        out.append(make_case(rng, n, m, ks(), "dup", rperp=r))
    t = 0
    for theta in (1e-2, 1e-3, 1e-4):
        for pair in ("pp", "pn", "eq"):
            for qn in (1.0, 1e2, 1e4, 1e5):
                if cell in ("wide_c5", "wide_pivoted", "wide_stage", "mid_overflow") and qn in (1e2, 1e4):
                    continue                         # (the big cells keep the extremes of |q~|)
                out.append(make_case(rng, n, m, ks(), "parallel", rperp=RPERP[t % 4], qnorm=qn, theta=theta, pair=pair))
                t += 1
    out.append(make_case(rng, n, m, ks(), "signforce"))
    out.append(make_case(rng, n, m, ks(), "signforce", qnorm=1e4))
    if batch:
        while len(out) < batch:
            out.append(make_case(rng, n, m, ks(), ("generic", "scale", "dup")[len(out) % 3], rperp=RPERP[len(out) % 4]))
    return out


MID_SLOTS = 256                                          # verify_wide_node's slots behind verify_node64 (QPN_VERIFY_MID_SLOTS)


def pad_node(rec, n_pad, m_pad):
    """The same node with n_pad more variables (x = 0, identity Hessian, untouched by the old rows) and m_pad more inactive
    one-hot rows on them: every sum the verify kernels form stays exact, so a padded exact case stays exact."""
    if not (n_pad or m_pad):
        return rec
    Q, R, qd, A, B, l, u, x, w = rec
    n, m = qd.shape[0], l.shape[0]
    N, M = n + n_pad, m + m_pad
    Q2 = np.eye(N); Q2[:n, :n] = Q
    R2 = np.zeros((N, R.shape[1])); R2[:n] = R
    A2 = np.zeros((M, N)); A2[:m, :n] = A
    for j in range(m_pad):
        A2[m + j, n + j % n_pad] = 1.0
    B2 = np.zeros((M, B.shape[1])); B2[:m] = B
    l2 = np.concatenate([l, np.full(m_pad, -0.5)]); u2 = np.concatenate([u, np.full(m_pad, 0.5)])
    return (Q2, R2, np.concatenate([qd, np.zeros(n_pad)]), A2, B2, l2, u2, np.concatenate([x, np.zeros(n_pad)]), w)
