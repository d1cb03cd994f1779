"""Records and hints for the warm start of block principal pivoting in the large class (QPN_OPT_WARM_BIG): shared
by tests/test_warm_big_host.py (the numpy twin, level_batch.warm_big_host) and tests/test_gpu_warm_big.py (the kernel).

Records: P.synth_nodes(30_000 + n + m, 4, n, m) in three bound modes -- "plain" as drawn, "loose" (every bound 3 further out: few
active rows), "tight" (two-sided boxes of width <= 0.6 round a common point: most rows at a bound, more than the 112 the kernel's
tiles hold).  Hints are multiplier vectors [cnt, m]; only their signs matter."""
import numpy as np

import problems as P

CNT = 4
KMAX = 112          # BPP_KMAX


def records(n, m, mode, cnt=CNT):
    """-> ((Q, R, qd, A, B, l, u) in math layout, the shared w)"""
    seed = n + m
    g = np.random.default_rng(seed)
    Q, R, qd, A, B, l, u = P.synth_nodes(30_000 + seed, cnt, n, m)
    w = P.shared_params()
    if mode == "tight":
        x0 = g.standard_normal((cnt, n))
        s0 = np.einsum("bij,bj->bi", A, x0) + B @ w
        l = s0 - g.uniform(0.0, 0.3, s0.shape); u = s0 + g.uniform(0.0, 0.3, s0.shape)
    elif mode == "loose":
        l = l - 3.0; u = u + 3.0
    else:
        assert mode == "plain"
    return (Q, R, qd, A, B, l, u), w


def abi(rec):
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u = rec
    return (colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u)


def schur(rec, w):
    """The Schur problem of every node: s = S lam + c with S = A Q^-1 A' and c = B w - A Q^-1 (qd + R w) -> (S [cnt, m, m], c)."""
    Q, R, qd, A, B, l, u = rec
    w = np.asarray(w, dtype=np.float64)
    q = qd + (R @ w if w.ndim == 1 else np.einsum("bnp,bp->bn", R, w))
    Bw = B @ w if w.ndim == 1 else np.einsum("bmp,bp->bm", B, w)
    W = np.linalg.solve(Q, np.concatenate([np.swapaxes(A, 1, 2), q[:, :, None]], axis=2))
    S = A @ W[:, :, :-1]
    S = 0.5 * (S + np.swapaxes(S, 1, 2))
    return S, Bw - np.einsum("bmn,bn->bm", A, W[:, :, -1])


def moved(w, delta, seed=5):
    """w after a relative move of delta per entry"""
    return w * (1.0 + delta * np.random.default_rng(seed).standard_normal(np.shape(w)))


def per_node(w, cnt=CNT, seed=6):
    """one parameter vector per node round the shared one"""
    return w[None, :] + 0.3 * np.random.default_rng(seed).standard_normal((cnt, w.size))


# ---- wrong hints: each names a set that is not the solution's
def redrawn(lam, seed=7):
    """10 % of the rows get a side drawn anew (lower, upper, none)"""
    g = np.random.default_rng(seed)
    h = np.array(lam, dtype=np.float64)
    pick = g.random(h.shape) < 0.10
    h[pick] = g.integers(-1, 2, h.shape)[pick]
    return h


def all_lower(lam, l):
    """every row with a finite lower bound at it"""
    return np.where(np.isfinite(l), 1.0, 0.0) + 0.0 * lam


def flipped(lam):
    return -np.asarray(lam)


WRONG = ("redrawn", "all_lower", "flipped")


def wrong(kind, lam, l):
    return dict(redrawn=lambda: redrawn(lam), all_lower=lambda: all_lower(lam, l), flipped=lambda: flipped(lam))[kind]()


# ---- a seed within the cap but above the rank of S (n = 70 < 100 rows): S_AA is singular, the seeded attempt has to fail
def dependent(m, cnt=CNT, rows=100):
    h = np.zeros((cnt, m))
    h[:, :rows] = 1.0
    return h


# ---- hints that name nothing
def one_sided(rec):
    """The records with the upper bound of every even row at +inf, and a hint that names only those sides."""
    Q, R, qd, A, B, l, u = rec
    u = u.copy(); u[:, ::2] = np.inf
    h = np.zeros_like(l); h[:, ::2] = -1.0
    return (Q, R, qd, A, B, l, u), h
