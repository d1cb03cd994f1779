"""The cases of tests/test_irredundant_host.py and tests/test_gpu_irredundant.py: polyhedra whose redundant bounds are known, the
pieces the pruning is for, and a reference that shares no code with the twin (HiGHS, scipy.optimize.linprog).

planted(r0, d, seed): max(r0, d + 1) unit normals, row d = minus the sum of the first d, renormalised, so that the normals span the
space positively and the set is bounded; every row a'x <= 1, tangent to the unit ball, so every one of them is a facet.  Three rows
are appended: a copy of row 0; 0.5 (a_1 + a_2) <= 1, weakly redundant (it touches the set where rows 1 and 2 meet, if they do, and
is implied either way); a_3 <= 1.5, strictly redundant.  The answer: exactly the three appended upper bounds go, and of the two
equal rows the appended one (tested first) goes and row 0 stays.  Where max(r0, d + 1) < 4 the rows 1, 2, 3 are taken modulo the
number of facets (at (1, 1): two facets, x <= 1 and -x <= 1).

HAND: one polyhedron per rule of the method.  pieces(): the twin outputs of project_cases.CASES; the 1101-row piece of (64, 65, 2)
is replaced by the input of its first Fourier-Motzkin step (pin_multipliers' rows, 129 of them over the columns that are left):
the twin, numpy with a Python loop per pivot, would take minutes on 1101 rows, and no `slow` mark exists in this suite.

check_as_sets asks of a pruning (lr, ur) of {l <= A x <= u}: only removals; for every removed bound HiGHS's extreme of that row over
the FINAL pruned set passes the original bound by at most TAU (relative to max(1, |bound|)); for every kept finite bound of a row
that is no equality HiGHS over the final set with that bound relaxed is unbounded or passes the bound by more than 10 tol; a bound
whose HiGHS margin lies in [tol / 10, 10 tol] is left out, at most 2 % of a case's bounds.

TAU: the twin's worst violation of a removed bound over the planted family at (3, 2), (8, 4), (16, 8), (40, 12), seeds 0..29, the
hand cases and pieces() is TWIN_WORST = 5.329e-15 (measured on the CPU, at (40, 12); 0 on every piece); TAU = 1000 x that = 5.329e-12.  It is never tuned from GPU output -- the GPU
output is bit-equal to the twin's and is not sent through this check at all.  test_irredundant_host.py asserts that the twin's
worst is TWIN_WORST to within a factor of 2 either way."""
from __future__ import annotations

import functools

import numpy as np

INF = np.inf
TOL = 1e-8
TWIN_WORST = 5.329e-15
TAU = 1000 * TWIN_WORST
PLANTED_SHAPES = [(3, 2), (8, 4), (16, 8), (40, 12)]
OUTPUTS = ("status", "fail_row", "lr", "ur", "how", "ext", "lps", "iters")


def planted(r0, d, seed):
    """-> (A [r, d], l, u [r], the planted rows [3])."""
    rng = np.random.default_rng([23, r0, d, seed])
    nf = max(r0, d + 1)
    A = rng.standard_normal((nf, d))
    A /= np.linalg.norm(A, axis=1)[:, None]
    A[d] = -A[:d].sum(axis=0)
    A[d] /= np.linalg.norm(A[d])
    i1, i2, i3 = 1 % nf, 2 % nf, 3 % nf
    A = np.vstack([A, A[0], 0.5 * (A[i1] + A[i2]), A[i3]])
    u = np.ones(nf + 3); u[-1] = 1.5
    return A, np.full(nf + 3, -INF), u, [nf, nf + 1, nf + 2]


def planted_batch(shape, seeds):
    """-> (A [polys, r, d], l, u [polys, r])."""
    cases = [planted(*shape, s) for s in seeds]
    return tuple(np.stack([c[k] for c in cases]) for k in range(3))


def one_sided_batch(seed, polys, r, d):
    """Polytopes of r one-sided rows for the class boundaries (r > d + 1): unit normals tangent to the unit ball, the first d + 1
    spanning the space positively; from row d + 1 on every third row is implied by earlier ones, in turn a_t'x <= 1.5 (strictly)
    and 0.5 (a_t + a_{t+1})'x <= 1 (weakly), t = 0, 1, ..."""
    rng = np.random.default_rng([29, seed, r, d])
    A = rng.standard_normal((polys, r, d))
    A /= np.linalg.norm(A, axis=2)[:, :, None]
    A[:, d] = -A[:, :d].sum(axis=1)
    A[:, d] /= np.linalg.norm(A[:, d], axis=1)[:, None]
    u = np.ones((polys, r))
    for t, k in enumerate(range(d + 1, r, 3)):
        if t % 2 == 0:
            A[:, k] = A[:, t]; u[:, k] = 1.5
        else:
            A[:, k] = 0.5 * (A[:, t] + A[:, t + 1])
    return A, np.full((polys, r), -INF), u


def implied_rows(r, d):
    return list(range(d + 1, r, 3))


# name -> (A, l, u); all 4 x 2 so that they go up as one batch
HAND = {
    # x0 == 1 exactly; the box rows of x0 are implied by it
    "equality": (np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0]]), np.array([1.0, -1.0, 0.0, -INF]), np.array([1.0, 1.0, 2.0, 3.0])),
    # 0'x in [-1, 1]
    "zero row": (np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [1.0, 1.0]]), np.array([-1.0, -1.0, -1.0, -INF]), np.array([1.0, 1.0, 1.0, 1.0])),
    # row 3: -5 <= x0 + x1 <= 1 over the unit box: the lower side is implied (the box reaches -2), the upper one cuts
    "one side": (np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0]]), np.array([-1.0, -1.0, -INF, -5.0]), np.array([1.0, 1.0, 5.0, 1.0])),
    # x1 has no upper bound but row 3's: KEPT_UNBOUNDED
    "unbounded": (np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0]]), np.array([-1.0, -1.0, -INF, -INF]), np.array([1.0, INF, 2.0, 4.0])),
    # x0 <= -1 and x0 >= 1
    "empty": (np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0]]), np.array([-INF, -1.0, 1.0, -INF]), np.array([-1.0, 1.0, INF, 3.0])),
    # l > u on row 0: no LP is started
    "crossed": (np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0]]), np.array([1.0, -1.0, -INF, -INF]), np.array([0.0, 1.0, 2.0, 3.0])),
}


def hand_batch():
    return tuple(np.stack([HAND[k][c] for k in HAND]) for c in range(3))


@functools.lru_cache(maxsize=None)
def pieces():
    """[(name, A [r, d], l, u)]: the twin outputs of project_cases.CASES, the columns no row reads left out; the 1101-row piece as the
    input of its first step."""
    import project_cases as pc
    from qpn_amd.avi_solutions import pin_multipliers
    out = []
    for name in pc.CASES:
        Ar, lr, ur, rows, flags = [np.asarray(a) for a in pc.twin_output(name)]
        n, m, p = pc.case(name)["shape"]
        for t in range(len(rows)):
            r = int(rows[t])
            if r > 1024:
                A, l, u, left = pin_multipliers(*pc.kept_rows(name, t), n, m)
                what = f"{name}/{t} (first step's input)"
            else:
                A, l, u = Ar[t].T[:r], lr[t][:r], ur[t][:r]
                what = f"{name}/{t}"
            cols = np.nonzero((A != 0).any(axis=0))[0]
            out.append((what, np.ascontiguousarray(A[:, cols]), np.array(l), np.array(u)))
    return out


def red_twin_engine():
    """tests/twin_engine.py's TwinEngine with the seventh entry served by its twin (a subclass: the engine itself stays as it is)."""
    from qpn_amd import polyhedra_host as ph
    from twin_engine import TwinEngine

    class RedTwinEngine(TwinEngine):
        def irredundant_bounds(self, Ac, l, u, tol=1e-8, opts=None):
            self._note("irredundant_bounds", Ac, l, u)
            return ph.irredundant_bounds_host(Ac, l, u, tol=tol, opts=opts)

    return RedTwinEngine()


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def highs_min(A, l, u, c):
    """min c'x over {l <= A x <= u} by HiGHS -> the optimum, -inf when unbounded, None when infeasible."""
    from scipy.optimize import linprog
    fu, fl = np.isfinite(u), np.isfinite(l)
    eq = fu & fl & (l == u)
    Aub = np.vstack([A[fu & ~eq], -A[fl & ~eq]]); bub = np.concatenate([u[fu & ~eq], -l[fl & ~eq]])
    for method, opts in (("highs", {}), ("highs-ds", {"presolve": False}), ("highs-ipm", {})):   # (status 4: HiGHS gave up; ask again)
        r = linprog(c, A_ub=Aub if len(bub) else None, b_ub=bub if len(bub) else None, A_eq=A[eq] if eq.any() else None,
                    b_eq=l[eq] if eq.any() else None, bounds=[(None, None)] * A.shape[1], method=method, options=opts)
        if r.status != 4:
            break
    if r.status == 3:
        return -INF
    if r.status == 2:
        return None
    assert r.status == 0, r.message
    return float(r.fun)


def check_as_sets(A, l, u, lr, ur, tol=TOL, tau=None, max_left_out=0.02):
    """-> (the worst relative violation of a removed bound over the final set, the bounds left out, the bounds asked)."""
    tau = TAU if tau is None else tau
    A, l, u, lr, ur = [np.asarray(a, dtype=np.float64) for a in (A, l, u, lr, ur)]
    assert np.all((lr == l) | (lr == -INF)) and np.all((ur == u) | (ur == INF)), "something other than a removal"
    worst, left_out, asked = 0.0, 0, 0
    for i in range(len(l)):
        for side, (b, now) in enumerate(((l[i], lr[i]), (u[i], ur[i]))):
            if not np.isfinite(b):
                continue
            sign = 1.0 if side == 0 else -1.0                     # min a'x against l, min -a'x against -u
            asked += 1
            if not np.isfinite(now):                              # removed: the final set stays within the bound
                v = highs_min(A, lr, ur, sign * A[i])
                assert v is not None, "the pruned set is empty"
                viol = (sign * b - v) / max(1.0, abs(b))
                worst = max(worst, viol)
                assert viol <= tau, (f"row {i} side {side}: a removed bound is passed by the pruned set", viol)
            elif l[i] != u[i]:                                    # kept: without it the final set passes it
                l2, u2 = lr.copy(), ur.copy()
                (l2 if side == 0 else u2)[i] = -INF if side == 0 else INF
                v = highs_min(A, l2, u2, sign * A[i])
                assert v is not None
                margin = (sign * b - v) / max(1.0, abs(b))
                if tol / 10 <= margin <= 10 * tol:
                    left_out += 1
                    continue
                assert margin > 10 * tol, (f"row {i} side {side}: a kept bound is implied by the others", margin)
    assert left_out <= max_left_out * asked, (left_out, asked)
    return worst, left_out, asked


def rows_left(lr, ur):
    return int(np.count_nonzero(np.isfinite(lr) | np.isfinite(ur)))


def same_bits(got, want, what):
    for k in OUTPUTS:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        w = np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.int64 if g.dtype == np.float64 else g.dtype) != w.view(np.int64 if w.dtype == np.float64 else w.dtype))
            raise AssertionError((what, k, "first difference at", bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])], len(bad)))


# ---- wrong methods: the checks have to catch them ---------------------------------------------------------------------------------
BUGS = ("all at once", "not restored", "tolerance reversed")


def irredundant_with(bug, A, l, u, tol=TOL):
    """polyhedra_host._irredundant_one restated with a switch, over the twin's own LP solves (bug = None: the same lr, ur):
      "all at once"         every bound is tested against the input set -- relaxed, solved, restored whatever the verdict -- and the
                            removals are applied together at the end: of two equal rows each is implied by the other, both go;
      "not restored"        a kept bound stays relaxed in the working bounds: the later tests run over a larger set;
      "tolerance reversed"  ext < l + tol max(1, |l|) (ext > u - tol ...) keeps the bound: a bound the set touches is kept.
    -> (lr, ur) of a polyhedron that ends OK."""
    from qpn_amd import polyhedra_host as ph
    A = np.ascontiguousarray(A, dtype=np.float64); l = np.array(l, dtype=np.float64); u = np.array(u, dtype=np.float64)
    o = dict(ph.LP_DEFAULT_OPTS)
    lw, uw = l.copy(), u.copy()
    status, S, _ = ph._lp_feasible(A, lw, uw, o)
    assert status == ph.LP_OPTIMAL
    gone = []
    for i in range(len(l) - 1, -1, -1):
        if l[i] == u[i]:
            continue
        if S.amax[i] == 0.0:
            gone += [(i, 0), (i, 1)]
            continue
        for side in (0, 1):
            bound = l[i] if side == 0 else u[i]
            if not abs(bound) < INF:
                continue
            ph._red_relax(S, lw, uw, i, side)
            status, _, obj = ph._lp_resolve(S, A[i].copy() if side == 0 else -A[i])
            assert status in (ph.LP_OPTIMAL, ph.LP_UNBOUNDED)
            margin = tol * max(1.0, abs(bound))
            if bug == "tolerance reversed":
                margin = -margin
            e = obj if side == 0 else -obj
            kept = status == ph.LP_UNBOUNDED or (e < bound - margin if side == 0 else e > bound + margin)
            if not kept:
                gone.append((i, side))
            if (kept and bug != "not restored") or (not kept and bug == "all at once"):
                ph._red_restore(S, lw, uw, i, side, bound)
    if bug == "not restored":
        return lw, uw
    lr, ur = l.copy(), u.copy()
    for i, side in gone:
        if side == 0:
            lr[i] = -INF
        else:
            ur[i] = INF
    return lr, ur
