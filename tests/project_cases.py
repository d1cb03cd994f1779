"""The cases of tests/test_project_pieces_host.py and tests/test_gpu_project_pieces.py: degenerate pieces (the ones qpn_reduced_pieces
flags), and a reference for their projection onto y = [x_d; x_p] that eliminates nothing.

Cases: the flagged pieces (a), (b), (c) of reduced_cases.degenerate for its FLAG_SHAPES; "pairs": two pairs of equal active rows in
one node, which leaves two columns, so the second Fourier-Motzkin step works on the first one's output; "scaled": an active row
and its double, where the step divides by 2 and the bounds are not 0 (the only case where an unscaled bound shows); "overflow": (64, 65, 2) (b)
with cap = n + 2m = 194, where the one step makes 1101 rows: flag 4 and all fill.

The reference: y is in the projection of the lifted piece {l <= A_y y + A_lam lam <= u} (local_pieces' rows) iff
    t*(y) = min t  s.t.  l - t <= A_y y + A_lam lam <= u + t,  t >= 0
is 0 -- an LP in (lam, t), solved by HiGHS (scipy.optimize.linprog).  Inside points are convex combinations of the y parts of
vertices of the lifted piece (random linear objectives over the piece cut with a box); the LP must confirm t* <= T_IN.  Outside
points are inside + 0.3 N(0,1) (off the manifold) and extrapolations on the affine hull -- from the vertices' centre along a
combination of (vertex - centre) to just behind the point where t* leaves 0, so that each leaves through one face --,
kept where t* >= MARGIN; a point with t* in between is skipped, at most 10 % of a case's points.  check_projection asks of an
engine's rows: inside points violate no row by more than TAU_IN (reduced_cases.violation, relative), outside points violate some
row by more than reduced_cases.TAU_OUT.  An empty lifted piece has no inside points: every drawn y is outside.

TAU_IN: the CPU twin (level_batch.project_pieces_host over OracleEngine.local_pieces) has a worst inside violation of 3.013e-15
over all cases (TWIN_WORST, at (40, 33, 3) (c); 1.9e-15 at (64, 65, 2) (c), at most 6.5e-16 at the (5, 6, 3) cases);
TAU_IN = 1000 x that = 3.013e-12.  The HIP engine meets the same constant; it is never tuned from GPU output.
test_project_pieces_host.py asserts that the twin's worst is TWIN_WORST to within a factor of 2 either way, so the constant cannot
drift away from what it is said to be."""
from __future__ import annotations

import functools

import numpy as np

import reduced_cases as rc

INF = np.inf
TWIN_WORST = 3.013e-15
TAU_IN = 1000 * TWIN_WORST
T_IN = 1e-12
BOX = 10.0
VERTS, DRAWS, RAYS = 6, 8, 8
OVERFLOW_ROWS = 1101          # what the one step of (64, 65, 2) (b) makes (test_overflow_case_is_what_it_says)


def _flagged(shape):
    d = rc.degenerate(shape)
    idx = np.nonzero(d["flags"])[0]
    return d, idx


def _scaled_case():
    """Node 0 of degenerate((5, 6, 3)) with row 1 := 2 x row 0 (A, B, l, u), rows 0, 1, 2 active: parallel active rows that are no
    copies, so the Fourier-Motzkin step divides by |a_j| = 2 and a bound that is not 0 -- where an unscaled bound shows."""
    shape = (5, 6, 3)
    n, m, p = shape
    Q, R, qd, A, B, l, u = [a[:1].copy() for a in rc.degenerate(shape)["rec"]]
    A[0, 1] = 2.0 * A[0, 0]; B[0, 1] = 2.0 * B[0, 0]; l[0, 1] = 2.0 * l[0, 0]; u[0, 1] = 2.0 * u[0, 0]
    K = np.full((1, n + m), 2, np.uint8); K[0, n:] = 6; K[0, n:n + 3] = 5
    return dict(shape=shape, args=rc.abi((Q, R, qd, A, B, l, u)), K=K, node_of=np.zeros(1, np.int32), names=["a doubled active row"])


def _pairs_case():
    """Node 0 of degenerate((5, 6, 3)) (rows 0, 1, 2 active at their lower bounds at a planted point) with row 1 := row 0 and
    row 3 := row 2, bit for bit, and the recipe that makes rows 0..3 active: two multiplier columns are left."""
    shape = (5, 6, 3)
    n, m, p = shape
    Q, R, qd, A, B, l, u = [a[:1].copy() for a in rc.degenerate(shape)["rec"]]
    for src, dst in ((0, 1), (2, 3)):
        A[0, dst] = A[0, src]; B[0, dst] = B[0, src]; l[0, dst] = l[0, src]; u[0, dst] = u[0, src]
    K = np.full((1, n + m), 2, np.uint8); K[0, n:] = 6; K[0, n:n + 4] = 5
    return dict(shape=shape, args=rc.abi((Q, R, qd, A, B, l, u)), K=K, node_of=np.zeros(1, np.int32), names=["two pairs of equal active rows"])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(shape, args (ABI layout), K, node_of, names, cap)."""
    from qpn_amd.level_batch import project_cap
    if name == "pairs":
        c = _pairs_case()
    elif name == "scaled":
        c = _scaled_case()
    else:
        shape = tuple(int(v) for v in name.split("-")[:3])
        d, idx = _flagged(shape)
        if name.endswith("overflow"):
            idx = np.array([t for t in idx if d["names"][t].startswith("b:")])
        c = dict(shape=shape, args=d["args"], K=d["K"][idx], node_of=d["node_of"][idx], names=[d["names"][t] for t in idx])
    n, m, p = c["shape"]
    # (64, 65, 2) (b) needs 1101 rows, more than project_cap gives it: the cases take room for it
    c["cap"] = n + 2 * m if name.endswith("overflow") else max(project_cap(n, m), 2048 if c["shape"] == (64, 65, 2) else 0)
    return c


CASES = ["5-6-3", "40-33-3", "64-65-2", "pairs", "scaled"]
OVERFLOW = "64-65-2-overflow"


@functools.lru_cache(maxsize=None)
def lifted(name):
    """local_pieces of the case on the CPU oracle: (Ap, lp, up, keep)."""
    from oracle_engine import OracleEngine
    c = case(name)
    return OracleEngine().local_pieces(*c["args"], c["K"], node_of=c["node_of"])


@functools.lru_cache(maxsize=None)
def twin_output(name):
    from qpn_amd.level_batch import project_pieces_host
    c = case(name)
    n, m, p = c["shape"]
    return project_pieces_host(*lifted(name), n, m, cap=c["cap"])


def kept_rows(name, t):
    Ap, lp, up, keep = lifted(name)
    rows = np.asarray(keep[t]).astype(bool)
    return np.asarray(Ap[t]).T[rows], np.asarray(lp[t])[rows], np.asarray(up[t])[rows]


# ---- the reference -------------------------------------------------------------------------------------------------------------
def _vertex(A, l, u, c):
    """argmin c.v over the lifted piece cut with |v| <= BOX, or None when it is empty."""
    from scipy.optimize import linprog
    fu, fl = np.isfinite(u), np.isfinite(l)
    eq = fu & fl & (l == u)
    Aub = np.vstack([A[fu & ~eq], -A[fl & ~eq]]); bub = np.concatenate([u[fu & ~eq], -l[fl & ~eq]])
    r = linprog(c, A_ub=Aub if len(bub) else None, b_ub=bub if len(bub) else None, A_eq=A[eq] if eq.any() else None,
                b_eq=l[eq] if eq.any() else None, bounds=[(-BOX, BOX)] * A.shape[1], method="highs")
    return r.x if r.status == 0 else None


def tstar(A, l, u, ycols, lcols, y):
    """min t >= 0 with l - t <= A_y y + A_lam lam <= u + t."""
    from scipy.optimize import linprog
    base = A[:, ycols] @ y
    fu, fl = np.isfinite(u), np.isfinite(l)
    Al = A[:, lcols]
    Aub = np.vstack([np.hstack([Al[fu], -np.ones((fu.sum(), 1))]), np.hstack([-Al[fl], -np.ones((fl.sum(), 1))])])
    bub = np.concatenate([u[fu] - base[fu], -(l[fl] - base[fl])])
    c = np.zeros(len(lcols) + 1); c[-1] = 1.0
    r = linprog(c, A_ub=Aub, b_ub=bub, bounds=[(None, None)] * len(lcols) + [(0, None)], method="highs")
    assert r.status == 0, r.message
    return float(r.x[-1])


@functools.lru_cache(maxsize=None)
def points(name):
    """Per piece of the case: dict(inside, outside [., n + p], empty, skipped, total)."""
    c = case(name)
    n, m, p = c["shape"]
    ycols = list(range(n)) + list(range(n + m, n + m + p)); lcols = list(range(n, n + m))
    rng = np.random.default_rng([17, n, m, p, len(name)])
    out = []
    for t in range(len(c["K"])):
        A, l, u = kept_rows(name, t)
        verts = [_vertex(A, l, u, rng.standard_normal(A.shape[1])) for _ in range(VERTS)]
        verts = [v for v in verts if v is not None]
        if not verts:
            cand = [rng.standard_normal(n + p) for _ in range(DRAWS)]
            ins = []
        else:
            V = np.array(verts)[:, ycols]
            ins = [rng.dirichlet(np.ones(len(V))) @ V for _ in range(DRAWS)]
            for y in ins:
                ts = tstar(A, l, u, ycols, lcols, y)
                assert ts <= T_IN, ("the LP does not confirm an inside point", name, t, ts)
            cand = [y + 0.3 * rng.standard_normal(n + p) for y in ins[:DRAWS // 2]]
            # extrapolations that leave the projection through ONE face each, so that every face is asked about on its own: from
            # the vertices' centre along a random combination of (vertex - centre), to just behind where t* leaves 0 (bisection)
            centre = V.mean(axis=0)
            for k in range(RAYS):
                d = rng.standard_normal(len(V)) @ (V - centre)
                if not np.any(d):
                    continue
                d /= np.linalg.norm(d)
                hi = 1.0
                while tstar(A, l, u, ycols, lcols, centre + hi * d) <= T_IN and hi < 1e3:
                    hi *= 2.0
                lo = 0.0
                for _ in range(12):
                    mid = 0.5 * (lo + hi)
                    if tstar(A, l, u, ycols, lcols, centre + mid * d) <= T_IN:
                        lo = mid
                    else:
                        hi = mid
                cand.append(centre + (hi + 0.02 * max(hi, 1.0)) * d)
        ts = np.array([tstar(A, l, u, ycols, lcols, y) for y in cand])
        keep = ts >= rc.MARGIN
        skipped = int(np.count_nonzero((ts > T_IN) & ~keep))
        # (an extrapolation that stays inside, t* <= T_IN, is an inside point)
        more_in = [y for y, s in zip(cand, ts) if s <= T_IN]
        out.append(dict(inside=np.array(ins + more_in).reshape(-1, n + p), outside=np.array(cand)[keep].reshape(-1, n + p),
                        empty=not verts, skipped=skipped, total=len(ins) + len(cand), tmin_out=float(ts[keep].min(initial=INF))))
    return out


def check_projection(out, pts, tau_in=TAU_IN):
    """The set-level check of an engine's output (Ar, lr, ur, rows, flags) on the case's points.  -> (worst inside violation,
    smallest outside violation)."""
    Ar, lr, ur, rows, flags = [np.asarray(a) for a in out]
    worst, least = 0.0, INF
    total = sum(q["total"] for q in pts); skipped = sum(q["skipped"] for q in pts)
    assert skipped <= 0.10 * total, (skipped, total)
    for t, q in enumerate(pts):
        assert flags[t] == 0, (t, int(flags[t]))
        assert q["empty"] or len(q["inside"]) >= DRAWS
        assert len(q["outside"]) >= 1, (t, "no outside point left")
        vin = rc.violation(Ar[t], lr[t], ur[t], rows[t], q["inside"])
        vout = rc.violation(Ar[t], lr[t], ur[t], rows[t], q["outside"])
        worst = max(worst, float(vin.max(initial=0.0))); least = min(least, float(vout.min(initial=INF)))
        assert vin.max(initial=0.0) <= tau_in, (f"piece {t}: a point of the projection is cut off", float(vin.max()))
        assert np.all(vout > rc.TAU_OUT), (f"piece {t}: a point outside the projection is let in", float(vout.min(initial=INF)))
    return worst, least


# ---- wrong eliminations: the check has to catch them ------------------------------------------------------------------------------
BUGS = ("pair dropped", "bounds not scaled", "upper and lower swapped")


def fourier_motzkin_with(bug, A, l, u, left, tol=1e-9):
    """avi_solutions.fourier_motzkin restated with a switch (bug = None: the same rows, bit for bit):
      "pair dropped"       the last (ub, lb) pair of a step is left out;
      "bounds not scaled"  the bounds of the one-sided inequalities are not divided by |a_j|;
      "upper and lower swapped"  a row's bounds change places: (a, l) and (-a, -u);
      "lists swapped"      every inequality goes to the other list.  This one is NOT a wrong elimination: every ub entry still
                           meets every lb entry and au + al = al + au bit for bit, so the same rows come out in another order --
                           the check cannot tell it from the right one, and need not."""
    A, l, u = np.array(A, dtype=np.float64), np.array(l, dtype=np.float64), np.array(u, dtype=np.float64)
    for j in left:
        zero = np.abs(A[:, j]) <= tol
        ub, lb = [], []
        for k in np.nonzero(~zero)[0]:
            lo_k, hi_k = (u[k], l[k]) if bug == "upper and lower swapped" else (l[k], u[k])
            for a_, b_ in ((A[k], hi_k), (-A[k], -lo_k)):
                if not np.isfinite(b_):
                    continue
                up = (a_[j] > 0) != (bug == "lists swapped")
                d = abs(a_[j])
                (ub if up else lb).append((a_ / d, b_ if bug == "bounds not scaled" else b_ / d))
        rows = [(au + al, bu + bl) for au, bu in ub for al, bl in lb]
        if bug == "pair dropped":
            rows = rows[:-1]
        A = np.vstack([A[zero]] + [r[0][None] for r in rows])
        l = np.concatenate([l[zero], np.full(len(rows), -INF)]); u = np.concatenate([u[zero], np.array([r[1] for r in rows])])
        A[:, j] = 0.0
    return A, l, u


def project_with(bug, name, t):
    """Piece t of the case through pin_multipliers and fourier_motzkin_with(bug) -> an output tuple of one piece for check_projection."""
    from qpn_amd.avi_solutions import pin_multipliers
    c = case(name)
    n, m, p = c["shape"]
    A, l, u, left = pin_multipliers(*kept_rows(name, t), n, m)
    A, l, u = fourier_motzkin_with(bug, A, l, u, left)
    ycols = [k for k in range(A.shape[1]) if k < n or k >= n + m]
    return A[:, ycols].T[None], l[None], u[None], np.array([A.shape[0]]), np.zeros(1, np.int32)
