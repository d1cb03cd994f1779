"""An independent reference for the reduced-Hessian convexity check: plain numpy, nothing of oracle/ and nothing of the product.

check_qp_convexity (src/qp_processing.jl:39-55) asks for lambda_min(Z' (Qd + Qd') Z) with Z an orthonormal basis of the null space
of the implicit equality rows Ae.  The kernel and the numpy restatement (test_convexity_host.convexity_restated) both DECIDE the
rank of Ae by a threshold; here the rank is GIVEN (the cases of tests/convexity_cases.py know it by construction), so the truth
does not depend on a rank rule:

reference   Z from a Householder QR with column pivoting of Ae' in np.longdouble (64-bit significand on x86; on a platform whose
            longdouble is narrower everything below still runs, with LD_EPS in the place of 2^-64, and the enclosures are wider),
            stopped after `rank` steps; H = Z' (Qd + Qd') Z in longdouble.  The answer is an ENCLOSURE [lam_lo, lam_hi] of
            lambda_min(H): the upper end is a Rayleigh quotient (>= lambda_min for any vector; the vector is numpy's float64
            eigenvector, the quotient is taken in longdouble), the lower end the largest tried shift hi - delta at which a
            longdouble Cholesky of H - (hi - delta) I completes (delta from 2^-60 |H|, doubled until it does), less the rounding
            a completed Cholesky can hide.
plain64     the float64 restatement (SVD, Vt[rank:], eigvalsh) with the same given rank: the "CPU oracle" whose error on a cell,
            E_ref, the kernel's accuracy bar is derived from (accuracy_bar, after solve_ref.accuracy_bar).
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
LD_EPS = float(np.finfo(LD).eps)
DELTA0 = max(2.0 ** -60, 16 * LD_EPS)     # first shift below the Rayleigh quotient, relative to |H|
FACTOR = 16                               # a kernel may be this many times worse than plain64 on the same cell ...
FLOOR = 64 * EPS                          # ... or this far from the enclosure (times |S|_2), whichever is larger
UNDERFLOW = 2.0 ** -1000                  # absolute: far below anything a case plants (the 2^-100 copies are at 1e-30)
OLD_BAR = 1e-9                           # test_gpu_convexity's tolerance (times max(1, |S|_2)): no bar may exceed it


def _ld(a):
    return np.asarray(a, dtype=LD)


def selected_rows(A, eq):
    """The rows the check reads: marked in eq and not all zero (an all-zero row constrains nothing)."""
    A = np.asarray(A, dtype=np.float64)
    if A.shape[0] == 0:
        return A
    return A[np.asarray(eq, dtype=bool) & np.any(A != 0, axis=1)]


def _house(x):
    """(v, tau) with (I - tau v v') x = beta e_1, in longdouble."""
    v = x.copy()
    sig = np.sum(x[1:] * x[1:])
    if sig == 0:
        v[0] = 1
        return v, LD(0)
    nrm = np.sqrt(x[0] * x[0] + sig)
    beta = -nrm if x[0] >= 0 else nrm
    v = x / (x[0] - beta)
    v[0] = 1
    return v, (beta - x[0]) / beta


def null_basis(Ae_rows, n, rank):
    """Z (n x (n - rank), longdouble): the last n - rank columns of Q of the column-pivoted Householder QR of Ae', stopped
    after `rank` steps.  The rows' common power-of-two scale is taken out first (exact; Z does not depend on it)."""
    Z = np.eye(n, dtype=LD)
    if rank == 0:
        return Z
    V = _ld(Ae_rows).T.copy()
    big = float(np.max(np.abs(V)))
    V = V * LD(2.0) ** -int(np.floor(np.log2(big)))
    for j in range(rank):
        norms = np.sum(V[j:, j:] * V[j:, j:], axis=0)
        pc = j + int(np.argmax(norms))
        assert norms[pc - j] > 0, "the given rank exceeds the rows' rank"
        V[:, [j, pc]] = V[:, [pc, j]]
        v, tau = _house(V[j:, j])
        if tau != 0:
            V[j:, j:] -= tau * np.outer(v, v @ V[j:, j:])
            Z[:, j:] -= tau * np.outer(Z[:, j:] @ v, v)
    return Z[:, rank:]


def _cholesky_completes(M):
    """Does a longdouble Cholesky of M run to the end with positive pivots?"""
    M = M.copy()
    d = M.shape[0]
    for j in range(d):
        p = M[j, j]
        if not p > 0:
            return False
        c = M[j + 1:, j] / p
        M[j + 1:, j + 1:] -= np.outer(c, M[j + 1:, j])
    return True


def reduced_hessian(Qd, Ae_rows, rank):
    n = Qd.shape[0]
    Z = null_basis(Ae_rows, n, rank)
    H = Z.T @ (_ld(Qd) + _ld(Qd).T) @ Z
    return 0.5 * (H + H.T)


def reference(Qd, Ae_rows, rank):
    """-> (lam_lo, lam_hi, null_dim): lam_lo <= lambda_min(Z' (Qd + Qd') Z) <= lam_hi, both longdouble (rounding them to float64
    would cost an ulp of lambda each, more than the whole enclosure); (+inf, +inf, 0) when the rows span everything."""
    Qd = np.asarray(Qd, dtype=np.float64)
    n = Qd.shape[0]
    d = n - rank
    if d == 0:
        return LD(np.inf), LD(np.inf), 0
    H = reduced_hessian(Qd, Ae_rows, rank)
    if not np.any(H != 0):
        return LD(0), LD(0), d
    s = LD(2.0) ** -int(np.floor(np.log2(float(np.max(np.abs(H))))))       # exact scaling: eigh sees entries of order one
    H64 = np.asarray(H * s, dtype=np.float64)
    norm = LD(np.linalg.norm(H64, 2)) * (1 + LD(2.0) ** -40) / s          # |H|_2, rounded up
    w, U = np.linalg.eigh(H64)
    v = _ld(U[:, 0])
    # the quotient's own rounding, |fl(v'Hv) - v'Hv| <= 2 d u |H| |v|^2 to first order: added, so that hi stays an upper bound
    hi = (v @ (H @ v)) / (v @ v) + 2 * d * LD_EPS * norm
    delta = LD(DELTA0) * norm
    eye = np.eye(d, dtype=LD)
    while not _cholesky_completes(H - (hi - delta) * eye):
        delta = 2 * delta
    # a completed Cholesky proves H - shift I + E positive definite with |E| <= (d + 1) u |H|: the shift less that is a bound
    lo = hi - delta - 2 * (d + 2) * LD_EPS * norm
    return lo, hi, d


def plain64(Qd, Ae_rows, rank):
    """The float64 restatement with the rank given: Z = Vt[rank:]' of the full SVD, eigvalsh of Z' (Qd + Qd') Z
    -> (min_eig, null_dim)."""
    Qd = np.asarray(Qd, dtype=np.float64)
    n = Qd.shape[0]
    if n - rank == 0:
        return np.inf, 0
    if rank:
        Ae = np.asarray(Ae_rows, dtype=np.float64)
        Ae = Ae * 2.0 ** -int(np.floor(np.log2(np.max(np.abs(Ae)))))      # (exact; LAPACK's SVD is not meant to be tested here)
        Z = np.linalg.svd(Ae, full_matrices=True)[2][rank:].T
    else:
        Z = np.eye(n)
    H = Z.T @ (Qd + Qd.T) @ Z
    return float(np.linalg.eigvalsh(0.5 * (H + H.T)).min()), n - rank


def dist(x, lo, hi):
    """distance of x from [lo, hi], taken in longdouble"""
    x = LD(x)
    return float(max(LD(lo) - x, x - LD(hi), LD(0)))


def accuracy_bar(e_ref, snorm, factor=FACTOR):
    """The bar the kernel's distance from the enclosure is held to on a node with |S|_2 = snorm.  e_ref: plain64's worst distance
    over |S|_2 on the same cell (relative, so that the cell's 2^+-100 copies do not set the bar of the unscaled nodes).  16: the
    kernel's QR, two-sided updates and tridiagonalisation sum in another order than LAPACK's blocked code; the floor is
    64 eps |S|_2, the few ulps of |S| that a backward-stable eigenvalue of S + E, |E| ~ n eps |S|, is good to.  UNDERFLOW: the
    Sturm count replaces a vanishing pivot by the smallest normal number, so an S of all zeros is answered to that, not to 0."""
    return max(factor * e_ref, FLOOR) * snorm + UNDERFLOW
