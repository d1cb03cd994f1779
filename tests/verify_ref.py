"""An independent CPU reference for verify_solution (src/qp_processing.jl:57-149), the accept gate that
csrc/qpn_verify.hip and oracle/qpn_oracle.c::qpo_verify_solution restate.

It does not copy either implementation's least squares.  From the exact float64 inputs it decides

    r* = min || A_bar lam - q~ ||_2  over sign-feasible lam   (>= 0 on pos and neg columns, free on both columns)

and returns r* as an interval [r_lo, r_hi]:

* every inner product of the inputs (q~ = Qd x + R w + qd, ax = Ad x + B w, residuals, A_bar' mu) is evaluated exactly and
  rounded once (error-free products + math.fsum); q~ is kept as a double-double;
* r_hi is the exactly evaluated residual of a sign-feasible lam (scipy's BVLS on the power-of-two equilibrated A_bar, its free
  set re-solved with iterative refinement on exact residuals); never the normal equations;
* r_lo comes from weak duality: for a unit mu with A_bar' mu <= 0 on the sign-constrained columns and = 0 on the free ones,
  r* >= <mu, q~>.  mu is the residual at the reference optimum (orthogonal to the optimum's free set by construction, KKT
  gives the signs elsewhere).  What is left of A_bar' mu on the columns it must vanish on is a rounding defect d (at most a few
  ulps of |mu|, evaluated exactly); its effect <d, lam> is charged against the bound for every multiplier vector within four
  times the reference's (plus 1), which is where a minimiser lies whenever the interval is narrow enough to decide anything.

certificate() checks a multiplier vector that a kernel returned, exactly, against the accept test it claims to have passed.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

EPS = 2.0 ** -53                     # unit roundoff of float64
FEAS_TOL, ACT_TOL, FALLBACK_TOL = 1e-3, 1e-2, 1e-4        # :86 (src/sets.jl), :98-99, :138
_SPLIT = 134217729.0                 # 2^27 + 1 (Veltkamp)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """Elementwise p + e == a * b exactly (Dekker; no overflow or underflow at this project's magnitudes)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def xmatvec(M, v, extra=None, dd=False):
    """Each entry of M @ v (+ extra[:, j] summed in) rounded once from the exact value.  dd=True: also the (exact-rounded)
    remainder, i.e. a double-double."""
    M = np.asarray(M, dtype=np.float64)
    if M.size == 0:
        hi = np.zeros(M.shape[0]) if extra is None else np.array([math.fsum(r) for r in np.atleast_2d(extra)])
        return (hi, np.zeros_like(hi)) if dd else hi
    P, E = two_prod(M, np.asarray(v, dtype=np.float64)[None, :])
    rows = np.concatenate([P, E] + ([np.asarray(extra, dtype=np.float64)] if extra is not None else []), axis=1)
    hi = np.array([math.fsum(r) for r in rows])
    if not dd:
        return hi
    lo = np.array([math.fsum(np.append(r, -h)) for r, h in zip(rows, hi)])
    return hi, lo


def xdot(a, b):
    p, e = two_prod(a, b)
    return math.fsum(np.concatenate([p.ravel(), e.ravel()]))


def xnorm(v):
    """||v||_2 with the sum of squares rounded once (then one sqrt: relative error <= 2 eps)."""
    return math.sqrt(max(xdot(v, v), 0.0))


@dataclass
class VerifyRef:
    feasible: bool
    cls: np.ndarray                  # per row: 0 inactive, 1 pos, 2 neg, 3 both (:98-103)
    margin: np.ndarray               # per row: distance of ax to the nearest threshold it is compared with (exact ax)
    ax: np.ndarray                   # exact ax, rounded once
    qt: np.ndarray                   # q~ (double-double: qt + qt_lo)
    qt_lo: np.ndarray
    cols: np.ndarray = field(default_factory=lambda: np.zeros(0, int))     # rows of A_bar's columns, order [pos | neg | both]
    k: int = 0
    r_lo: float = 0.0
    r_hi: float = 0.0
    lam: np.ndarray = None           # sign-feasible multipliers (kernel convention: lam[neg] <= 0) achieving r_hi
    cond_eq: float = 1.0             # cond of A_bar with unit columns, duplicate columns (up to sign) counted once
    path: int = None                 # the path the reference predicts when it is unambiguous (0, 1, 2, 3, 4), else None

    def decided(self, thr):
        """True / False when the interval lies on one side of thr, None when it straddles."""
        if self.r_hi <= thr:
            return True
        if self.r_lo > thr:
            return False
        return None


def _exact_inputs(Qd, R, qd, Ad, B, xd, w):
    Qd, R, qd, Ad, B, xd, w = (np.asarray(a, dtype=np.float64) for a in (Qd, R, qd, Ad, B, xd, w))
    n = qd.shape[0]
    m = Ad.shape[0] if Ad.size else 0
    p = w.shape[0]
    Rw = two_prod(R.reshape(n, p), w[None, :]) if p else (np.zeros((n, 0)), np.zeros((n, 0)))
    qt, qt_lo = xmatvec(Qd.reshape(n, n), xd, extra=np.concatenate([Rw[0], Rw[1], qd[:, None]], axis=1), dd=True)
    if m:
        A = Ad.reshape(m, n)
        Bw = two_prod(B.reshape(m, p), w[None, :]) if p else (np.zeros((m, 0)), np.zeros((m, 0)))
        ax = xmatvec(A, xd, extra=np.concatenate([Bw[0], Bw[1]], axis=1))
    else:
        A, ax = np.zeros((0, n)), np.zeros(0)
    return A, qt, qt_lo, ax


def classify(ax, l, u):
    """Feasibility (:86 with the kernels' expression of Slice membership) and the classes of :98-103, evaluated on the exact
    ax as the reference evaluates them on its ax: l - 1e-3 <= ax and ax - 1e-3 <= u; ax < l + 1e-2 (pos), ax > u - 1e-2 (neg)."""
    l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        feas = bool(np.all((l - FEAS_TOL <= ax) & (ax - FEAS_TOL <= u)))
        pos = ax < l + ACT_TOL
        neg = ax > u - ACT_TOL
        th = np.stack([l + ACT_TOL, u - ACT_TOL, l - FEAS_TOL, u + FEAS_TOL])
        d = np.abs(th - ax[None, :])
        d[~np.isfinite(d)] = np.inf
    cls = pos.astype(np.int8) + 2 * neg.astype(np.int8)
    return feas, cls, d.min(axis=0) if ax.size else np.zeros(0)


def _abar(A, cls):
    cols = np.concatenate([np.flatnonzero(cls == 1), np.flatnonzero(cls == 2), np.flatnonzero(cls == 3)]).astype(int)
    sg = np.where(cls[cols] == 2, -1.0, 1.0)
    return cols, A[cols].T * sg[None, :], cls[cols] != 3


def _pow2_scale(Ab):
    """Column scales 2^e with every column's norm in [0.5, 1): A_bar * s is exact."""
    nr = np.linalg.norm(Ab, axis=0)
    e = np.where(nr > 0, -np.floor(np.log2(np.where(nr > 0, nr, 1.0))) - 1, 0.0)
    return np.ldexp(1.0, e.astype(int))


def _cond_eq(Ae):
    if Ae.shape[1] == 0:
        return 1.0
    Un = Ae / np.linalg.norm(Ae, axis=0)[None, :]
    keep = []
    for j in range(Un.shape[1]):                  # drop exact duplicates up to sign
        if not any(np.array_equal(Un[:, j], Un[:, i]) or np.array_equal(Un[:, j], -Un[:, i]) for i in keep):
            keep.append(j)
    s = np.linalg.svd(Un[:, keep], compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else math.inf


def _residual(Ab, lam, qt, qt_lo, lam_lo=None):
    """q~ - A_bar (lam + lam_lo), each entry rounded once from the exact value."""
    if Ab.size == 0:
        return np.array([math.fsum(r) for r in zip(qt, qt_lo)])
    parts = [qt[:, None], qt_lo[:, None]]
    for lv in (lam,) if lam_lo is None else (lam, lam_lo):
        P, E = two_prod(Ab, lv[None, :])
        parts += [-P, -E]
    rows = np.concatenate(parts, axis=1)
    return np.array([math.fsum(r) for r in rows])


def _bounded_lsq(Ae, qt, qt_lo, con):
    """Sign-feasible least squares on the equilibrated columns: BVLS, then its free set re-solved and refined on exact
    residuals with the correction kept apart (lam + lam_lo, a double-double: the residual of a lam rounded to doubles is
    orthogonal to the free columns only to eps |A_bar| |lam|, which is far from |r*| when |q~| or cond are large).  Returns
    (lam, lam_lo), sign-feasible."""
    from scipy.optimize import lsq_linear
    k = Ae.shape[1]
    lb = np.where(con, 0.0, -np.inf)
    res = lsq_linear(Ae, qt, bounds=(lb, np.full(k, np.inf)), method="bvls", tol=1e-15, max_iter=50 * k + 100)
    lam = np.where(con, np.maximum(res.x, 0.0), res.x)
    zero = np.zeros(k)
    best = (xnorm(_residual(Ae, lam, qt, qt_lo)), lam, zero)
    free = (~con) | (lam > 0)
    if free.any():
        # an independent subset of the free set, heaviest columns first (dependent columns -- duplicates, a row both pos and
        # neg -- would let the minimum-norm solution split their weight across opposite signs)
        order = np.flatnonzero(free)[np.argsort(-np.abs(lam[free]), kind="stable")]
        rd = np.abs(np.diag(np.linalg.qr(Ae[:, order], mode="r")))
        free = np.zeros(k, bool)
        free[order[rd > 1e-9 * max(rd.max(), 1e-300)]] = True
        Af = Ae[:, free]
        hi = np.zeros(k); lo = np.zeros(k)
        hi[free] = np.linalg.lstsq(Af, qt, rcond=None)[0]
        for it in range(4):
            r = _residual(Ae, hi, qt, qt_lo, lo)
            d = np.zeros(k); d[free] = np.linalg.lstsq(Af, r, rcond=None)[0]
            if it == 0:
                hi = hi + d                       # (the first correction still moves the leading digits)
            else:
                lo = lo + d
        s = hi + lo
        hi, lo = s, lo - (s - hi)                 # renormalise (Fast2Sum: |hi| >= |lo|)
        if np.all(hi[con] >= 0):
            r2 = xnorm(_residual(Ae, hi, qt, qt_lo, lo))
            if r2 <= best[0]:
                best = (r2, hi, lo)
    return best[1], best[2]


def _lower_bound(Ae, lam, lam_lo, qt, qt_lo, con):
    """Weak duality with mu = q~ - A_bar lam at the reference optimum (see the module docstring)."""
    mu = _residual(Ae, lam, qt, qt_lo, lam_lo)
    nmu = xnorm(mu)
    if nmu == 0.0:
        return 0.0
    v = xmatvec(Ae.T, mu) if Ae.size else np.zeros(0)        # A_bar' mu, each entry rounded once
    bad = (~con) | (v > 0)                                     # where it has to vanish (free) or has the wrong sign
    lam_cap = 4.0 * np.abs(lam) + 1.0
    defect = float(np.sum(np.abs(v[bad]) * lam_cap[bad])) * (1 + 4 * EPS) + np.sum(np.abs(v[bad])) * 2 * EPS
    mq = xdot(mu, qt) + xdot(mu, qt_lo)                         # <mu, q~> (the second term: q~'s low part)
    err = 4 * EPS * (abs(mq) + nmu * float(np.linalg.norm(qt)) * 4 * EPS)
    return max(0.0, (mq - defect - err) / nmu * (1 - 8 * EPS))


def verify_reference(Qd, R, qd, Ad, B, l, u, xd, w, tol=1e-4) -> VerifyRef:
    """The decision of verify_solution at (xd, w) for one node record (math layout), as an interval on r*."""
    A, qt, qt_lo, ax = _exact_inputs(Qd, R, qd, Ad, B, xd, w)
    m = A.shape[0]
    feas, cls, margin = classify(ax, l, u)
    ref = VerifyRef(feasible=feas, cls=cls, margin=margin, ax=ax, qt=qt, qt_lo=qt_lo, lam=np.zeros(m))
    if not feas:
        ref.r_lo = ref.r_hi = math.inf
        ref.path = 0
        return ref
    cols, Ab, con = _abar(A, cls)
    ref.cols, ref.k = cols, len(cols)
    if ref.k == 0:
        r = xnorm(qt + qt_lo)
        ref.r_lo, ref.r_hi = r * (1 - 4 * EPS), r * (1 + 4 * EPS)
        ref.path = 1 if m == 0 else (2 if ref.r_hi <= tol else (4 if ref.r_lo > max(tol, FALLBACK_TOL) else None))
        return ref
    s = _pow2_scale(Ab)
    Ae = Ab * s[None, :]
    ref.cond_eq = _cond_eq(Ae)
    lam_e, lam_e_lo = _bounded_lsq(Ae, qt, qt_lo, con)
    ref.r_hi = xnorm(_residual(Ae, lam_e, qt, qt_lo, lam_e_lo)) * (1 + 4 * EPS)
    ref.r_lo = min(_lower_bound(Ae, lam_e, lam_e_lo, qt, qt_lo, con), ref.r_hi)
    lam_bar = lam_e * s
    lam = np.zeros(m)
    lam[cols] = np.where(cls[cols] == 2, -lam_bar, lam_bar)
    ref.lam = lam
    # the path, where the data leave no doubt about it: the unconstrained least squares (:115) of a full-rank A_bar with clear
    # signs and a clear residual decides :119; otherwise the bounded least squares decides :138
    if ref.cond_eq < 1e6 and np.linalg.matrix_rank(Ae) == ref.k:
        y, *_ = np.linalg.lstsq(Ae, qt, rcond=None)
        yb = y * s
        r_unc = xnorm(_residual(Ae, y, qt, qt_lo))
        sign_ok = bool(np.all(yb[con] > -tol + 1e-3 * tol)) if con.any() else True
        sign_bad = bool(np.any(yb[con] < -tol - 1e-3 * tol)) if con.any() else False
        if sign_ok and r_unc <= 0.5 * tol:
            ref.path = 2
        elif sign_bad or r_unc > 2 * tol:
            ref.path = 3 if ref.r_hi <= 0.5 * FALLBACK_TOL else (4 if ref.r_lo > 2 * FALLBACK_TOL else None)
    return ref


def certificate(lam, ref: VerifyRef, Ad, path, tol=1e-4, Qd=None, R=None, xd=None, w=None, qd=None):
    """Checks exactly that lam (length m, as a kernel returns it) certifies an accept on `path` (2: the test of :119 with `tol`;
    3: the test of :138 with 1e-4): zero on inactive rows, signs within tol on pos (>= -tol) and neg (<= tol) rows, and
    || Ad' lam - q~ || <= threshold + a rounding allowance derived from the operation counts (the kernels form q~ with n + p + 1
    terms and A_bar lam - q~ with k + 1 more).  Returns (ok, message)."""
    lam = np.asarray(lam, dtype=np.float64)
    Ad = np.asarray(Ad, dtype=np.float64)
    m, n = Ad.shape
    cls = ref.cls
    if np.any(lam[cls == 0] != 0.0):
        return False, f"nonzero multiplier on inactive rows {np.flatnonzero((cls == 0) & (lam != 0))}"
    if np.any(lam[cls == 1] < -tol) or np.any(lam[cls == 2] > tol):
        return False, "multiplier of the wrong sign"
    thr = tol if path == 2 else FALLBACK_TOL
    r = -_residual(Ad.T, lam, ref.qt, ref.qt_lo)               # Ad' lam - q~
    res = xnorm(r)
    # |q~|'s own terms: |Qd||x| + |R||w| + |qd| when given, else |q~|
    if Qd is not None:
        p = np.asarray(w).shape[0]
        qabs = np.abs(Qd) @ np.abs(xd) + (np.abs(np.asarray(R).reshape(n, p)) @ np.abs(w) if p else 0.0) + np.abs(qd)
        nq = n + p + 1
    else:
        qabs, nq = np.abs(ref.qt), 1
    k = max(ref.k, 1)
    gam = lambda t: t * EPS / (1 - t * EPS)
    allow = float(np.linalg.norm(gam(k + 2) * (np.abs(Ad.T) @ np.abs(lam)) + gam(nq + k + 2) * qabs)) * (1 + 8 * EPS)
    ok = res <= thr + allow
    return ok, f"||Ad' lam - q~|| = {res:.3e} vs {thr:.0e} + {allow:.1e}"
