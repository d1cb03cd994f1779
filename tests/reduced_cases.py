"""The cases of tests/test_reduced_pieces_host.py and tests/test_gpu_reduced_pieces.py: node records, recipes, and a reference for
qpn_reduced_pieces that shares nothing with the kernel's elimination -- plain numpy on the unscaled data.

A reduced piece is a SET over y = [x_d; x_p].  The reference decides membership of points without eliminating anything: for a
recipe it solves the KKT system of the recipe's active rows at a parameter draw w' (float64, two steps of iterative refinement
with long-double residuals), which puts y = [x_d; w'] on the recipe's equality manifold; y belongs to the piece iff the signs of
the active multipliers and the bounds of the inactive rows hold, and its margin is the smallest slack of those conditions.
check_piece then asks of the rows an engine returned: points inside by >= MARGIN violate no row by more than TAU_IN (relative to
scale_k = sum_i |a_ki| |y_i| + |finite bounds of row k|), points outside by >= MARGIN violate some row by more than TAU_OUT, and
points pushed off the manifold (x_d + 1e-4 N(0,1)) violate some row by more than TAU_OFF.

TAU_IN: the CPU twin (tests/oracle_engine.py::OracleEngine.reduced_pieces) over every case of CASES has a worst inside violation
of 3.654e-16 (shape (256, 256, 2), kind box; at most 3.4e-16 at every other case, whatever its size).  TAU_IN = 1000 x that = 3.65e-13, below the cap of 1e-11.  The HIP engine meets the same constant; it is never tuned from
GPU output.  TAU_OUT = 1e-9: outside points sit at least 1e-6 off a face.

Class balance per case (asserted by check_balance): at most 10 % of the points may be skipped as nearer than MARGIN to a face,
and inside and outside each hold at least 20 % of the rest.  With m = 0 a piece is its equality manifold and nothing else, so no
point on the manifold can be outside: there the outside class is empty by construction and the off-manifold points stand in."""
from __future__ import annotations

import functools

import numpy as np

import problems as P

INF = np.inf
TAU_IN = 3.65e-13
TAU_OUT = 1e-9
TAU_OFF = 1e-7
MARGIN = 1e-6
SCALES = (0.0, 1e-3, 0.05, 0.3, 1.0)
KINDS = ("gauss", "mixed", "box")

# (n, m, p): the smallest shapes that reach each path of reduce_pieces_kernel (its loops stride by 256 over 2 (n + m) rows)
SHAPES = [(5, 6, 3), (7, 0, 2), (3, 4, 0), (32, 32, 8), (40, 33, 3),
          (64, 64, 2),       # 256 rows: exactly one stride
          (64, 65, 2),       # 258 rows: the first second stride
          (100, 130, 2), (129, 129, 2),
          (256, 256, 2)]     # the limit: four rows per thread
CASES = [(s, k) for s in SHAPES for k in KINDS if k != "mixed" or s[0] + s[1] <= 129]
FLAG_SHAPES = [(5, 6, 3), (40, 33, 3), (64, 65, 2)]
NODES = 2
# seeds that differ from the default 0 (a seed is changed when a case misses check_balance's caps; the caps never move)
SEEDS = {}


def case_id(c):
    (n, m, p), kind = c
    return f"{n}-{m}-{p}-{kind}"


def colmajor(M):
    """(..., rows, cols) math layout -> the ABI's column-major layout (what the engine and OracleEngine take)."""
    return np.ascontiguousarray(np.swapaxes(np.asarray(M, dtype=np.float64), -1, -2))


def abi(rec):
    Q, R, qd, A, B, l, u = rec
    return colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u


def base_w(p):
    return P.shared_params(p)


def records(shape, kind, seed=0, nodes=NODES):
    """Node records (Q, R, qd, A, B, l, u) in math layout, `nodes` of them.
    gauss: synth_nodes with B = 0.2 N(0,1).  mixed: gauss with about 15 % of the rows lower-only, 15 % upper-only, 5 % free and a
    few l == u.  box (the ties case): the first min(n, m) rows of A are e_i in [-0.3, 0.3]; where m > n the next rows are -e_i
    with bounds of their own; any further rows stay Gaussian."""
    n, m, p = shape
    Q, R, qd, A, B, l, u = P.synth_nodes(300 + 16 * seed, nodes, n, m, p)
    g = np.random.default_rng([seed, n, m, p, KINDS.index(kind)])
    B = 0.2 * g.standard_normal((nodes, m, p))
    if kind == "mixed":
        c = g.random((nodes, m))
        l = np.where((c >= 0.15) & (c < 0.35), -INF, l)                 # upper-only [0.15, 0.30), free [0.30, 0.35)
        u = np.where((c < 0.15) | ((c >= 0.30) & (c < 0.35)), INF, u)   # lower-only [0, 0.15)
        for b in range(nodes):
            for k in g.choice(m, min(m, max(1, m // 16)), replace=False) if m else ():
                l[b, k] = u[b, k] = 0.3 * g.standard_normal()
    elif kind == "box":
        k1 = min(n, m)
        A[:, :k1] = 0.0
        A[:, np.arange(k1), np.arange(k1)] = 1.0
        l[:, :k1] = -0.3; u[:, :k1] = 0.3
        k2 = min(n, m - k1)
        A[:, k1:k1 + k2] = 0.0
        A[:, k1 + np.arange(k2), np.arange(k2)] = -1.0
        l[:, k1:k1 + k2] = -0.5; u[:, k1:k1 + k2] = 0.2                 # x_i in [-0.2, 0.5]: with the first rows, [-0.2, 0.3]
    return Q, R, qd, A, B, l, u


def solve_node(rec, b, w):
    """The node's solution z = [x_d; lambda] at parameters w on the CPU oracle (math layout in), checked for stationarity."""
    from oracle import binding as ob
    Q, R, qd, A, B, l, u = [a[b] for a in rec]
    n, m = Q.shape[0], A.shape[0]
    if m == 0:
        return np.linalg.solve(Q, -(qd + R @ w))
    M, q, lo, hi, kind = ob.assemble_node(Q, R, qd, A, B, l, u, w)
    res = ob.solve_avi_batch(M[None], q[None], lo[None], hi[None], kind=kind[None])
    assert int(res["status"][0]) == ob.SUCCESS
    z = res["z"][0]
    x, lam = z[:n], z[n:]
    assert np.max(np.abs(Q @ x - A.T @ lam + R @ w + qd)) <= 1e-9 * (1.0 + np.max(np.abs(z))), "stationarity: wrong layout?"
    return z


def recipes(rec, w, neighbours=2):
    """-> K [pieces, n + m] uint8, node_of [pieces] int32, strict [pieces] bool (the node's own recipe).  Per node: the strict
    recipe of the oracle's solution (x rows code 2; lambda > 1e-9 -> 5, < -1e-9 -> 7, else 6); up to `neighbours` recipes that
    differ from it in one row -- the inactive row nearest to a finite bound made active there (the nearest one that keeps the
    active rows independent), and the active row with the smallest multiplier made inactive --; and, where the node has a row
    with l == u, the strict recipe with code 8 on the first such row."""
    Q, R, qd, A, B, l, u = rec
    nodes, n = qd.shape
    m = l.shape[1]
    Ks, node_of, strict = [], [], []
    for b in range(nodes):
        z = solve_node(rec, b, w)
        x, lam = z[:n], z[n:]
        K = np.full(n + m, 2, np.uint8)
        K[n:] = np.where(lam > 1e-9, 5, np.where(lam < -1e-9, 7, 6))
        mine = [K]
        eq = l[b] == u[b]
        act = np.nonzero((K[n:] != 6) & ~eq)[0]
        inact = np.nonzero((K[n:] == 6) & ~eq & (np.isfinite(l[b]) | np.isfinite(u[b])))[0]
        if neighbours >= 1 and len(inact) and np.count_nonzero(K[n:] != 6) < n:
            s = A[b] @ x + B[b] @ w
            slack = np.minimum(s - l[b], u[b] - s)[inact]
            on = np.nonzero(K[n:] != 6)[0]
            for k in inact[np.argsort(slack)]:                          # (the box case: not -e_i next to an active e_i)
                if np.linalg.matrix_rank(A[b][np.append(on, k)]) == len(on) + 1:
                    Kn = K.copy(); Kn[n + k] = 5 if s[k] - l[b, k] <= u[b, k] - s[k] else 7
                    mine.append(Kn)
                    break
        if neighbours >= 2 and len(act):
            k = int(act[np.argmin(np.abs(lam[act]))])
            Kn = K.copy(); Kn[n + k] = 6
            mine.append(Kn)
        if eq.any():
            Kn = K.copy(); Kn[n + int(np.nonzero(eq)[0][0])] = 8
            mine.append(Kn)
        Ks += mine; node_of += [b] * len(mine); strict += [True] + [False] * (len(mine) - 1)
    return np.array(Ks, np.uint8).reshape(len(Ks), n + m), np.array(node_of, np.int32), np.array(strict)


def reference_points(rec, K_t, b, rng, w=None, draws=4):
    """Points of known membership for the piece of recipe K_t on node b (see the module docstring).
    -> dict(inside, outside, off [., n + p], skipped, total, resid)."""
    Q, R, qd, A, B, l, u = [np.asarray(a[b], dtype=np.float64) for a in rec]
    n, m, p = Q.shape[0], A.shape[0], R.shape[1]
    w = base_w(p) if w is None else w
    code = np.asarray(K_t[n:], dtype=np.int64)
    if np.any(np.asarray(K_t[:n]) != 2):
        raise ValueError("reference_points: x rows carry code 2")
    free = ~np.isin(code, (5, 6, 7))
    empty = ~(np.abs(A) > 1e-8).any(axis=1) & ~(np.abs(B) > 1e-8).any(axis=1)      # rows that local_piece drops
    if np.any(free & (l != u) & ~empty) or np.any(~free & (code != 6) & empty):
        raise ValueError("reference_points: a free multiplier on a row with l < u, or an active empty row")
    act = np.nonzero((code == 5) | (code == 7) | (free & (l == u)))[0]
    inact = np.setdiff1d(np.arange(m), act)
    bnd = np.where(code[act] == 7, u[act], l[act])
    if not np.all(np.isfinite(bnd)):
        raise ValueError("reference_points: a row active at an infinite bound")
    na = len(act)
    W = np.concatenate([w[:, None] + s * rng.standard_normal((p, draws)) for s in SCALES], axis=1)
    Kmat = np.block([[Q, -A[act].T], [A[act], np.zeros((na, na))]])
    rhs = np.concatenate([-qd[:, None] - R @ W, bnd[:, None] - B[act] @ W])
    sol = np.linalg.solve(Kmat, rhs)
    KL, rl = Kmat.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(2):
        sol = sol + np.linalg.solve(Kmat, (rl - KL @ sol.astype(np.longdouble)).astype(np.float64))
    res = np.abs(rl - KL @ sol.astype(np.longdouble)).max(axis=0)
    den = np.abs(Kmat).sum(axis=1).max() * np.abs(sol).max(axis=0) + np.abs(rhs).max(axis=0)
    resid = float(np.max(res / den))
    assert resid <= 1e-13, resid                                       # the reference's own guard
    X, lam = sol[:n], sol[n:]
    slacks = [np.full((1, W.shape[1]), INF)]
    slacks.append(lam[code[act] == 5]); slacks.append(-lam[code[act] == 7])
    s = A[inact] @ X + B[inact] @ W
    slacks.append(s - l[inact][:, None]); slacks.append(u[inact][:, None] - s)
    margin = np.concatenate(slacks).min(axis=0)
    Y = np.concatenate([X, W]).T
    off = np.concatenate([X + 1e-4 * rng.standard_normal(X.shape), W]).T
    return dict(inside=Y[margin >= MARGIN], outside=Y[margin <= -MARGIN], off=off,
                skipped=int(np.count_nonzero(np.abs(margin) < MARGIN)), total=int(len(margin)), resid=resid)


def violation(Ar_t, lr_t, ur_t, rows_t, Y):
    """max over the rows k < rows_t of max(l_k - a_k y, a_k y - u_k, 0) / scale_k, for every point of Y [., n + p]."""
    r = int(rows_t)
    a = np.asarray(Ar_t, dtype=np.float64).T[:r]
    lo, hi = np.asarray(lr_t)[:r], np.asarray(ur_t)[:r]
    Y = np.asarray(Y, dtype=np.float64)
    if r == 0 or len(Y) == 0:
        return np.zeros(len(Y))
    ay = Y @ a.T
    scale = np.abs(Y) @ np.abs(a).T + np.where(np.isfinite(lo), np.abs(lo), 0.0) + np.where(np.isfinite(hi), np.abs(hi), 0.0)
    num = np.maximum(np.maximum(lo - ay, ay - hi), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(num > 0.0, num / scale, 0.0)                       # (a violated row of scale 0 counts as +inf)
    return v.max(axis=1)


def check_piece(Ar_t, lr_t, ur_t, rows_t, points, tau_in=TAU_IN):
    """The set-level check of one piece.  -> (worst inside violation, smallest outside violation, smallest off-manifold one)."""
    vin = violation(Ar_t, lr_t, ur_t, rows_t, points["inside"])
    vout = violation(Ar_t, lr_t, ur_t, rows_t, points["outside"])
    voff = violation(Ar_t, lr_t, ur_t, rows_t, points["off"])
    worst = float(vin.max(initial=0.0))
    assert worst <= tau_in, ("a point of the piece is cut off", worst)
    assert np.all(vout > TAU_OUT), ("a point outside the piece is let in", float(vout.min(initial=INF)))
    assert np.all(voff > TAU_OFF), ("a point off the equality manifold is let in", float(voff.min(initial=INF)))
    return worst, float(vout.min(initial=INF)), float(voff.min(initial=INF))


def check_pieces(out, points, flags_clear=True):
    """check_piece over every piece of an engine's output (Ar, lr, ur, rows, flags).  -> the worst inside violation."""
    Ar, lr, ur, rows, flags = [np.asarray(a) for a in out]
    worst = 0.0
    for t, pts in enumerate(points):
        assert not flags_clear or flags[t] == 0, (t, int(flags[t]))
        try:
            worst = max(worst, check_piece(Ar[t], lr[t], ur[t], rows[t], pts)[0])
        except AssertionError as e:
            raise AssertionError(f"piece {t}: {e}") from None
    return worst


def check_balance(shape, points):
    """The conditions on a case's points: <= 10 % skipped, inside and outside >= 20 % of the rest each (m = 0: no outside)."""
    total = sum(q["total"] for q in points); skipped = sum(q["skipped"] for q in points)
    ins = sum(len(q["inside"]) for q in points); out = sum(len(q["outside"]) for q in points)
    assert ins + out + skipped == total
    assert skipped <= 0.10 * total, (skipped, total)
    if shape[1] == 0:
        assert out == 0 and ins == total
    else:
        assert ins >= 0.20 * (total - skipped) and out >= 0.20 * (total - skipped), (ins, out, total)
    return ins, out, skipped


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """-> dict(rec (math layout), args (ABI layout), K, node_of, points [pieces]) of one (shape, kind), computed once."""
    seed = SEEDS.get((shape, kind), 0)
    rec = records(shape, kind, seed)
    w = base_w(shape[2])
    K, node_of, strict = recipes(rec, w)
    rng = np.random.default_rng([seed, 7] + list(shape))
    # the parameter draws land inside a node's own piece about half of the time and outside a neighbouring piece nearly always:
    # the own piece gets more draws, so that both classes are populated
    points = [reference_points(rec, K[t], int(node_of[t]), rng, w, draws=8 if strict[t] else 2) for t in range(len(K))]
    return dict(rec=rec, args=abi(rec), K=K, node_of=node_of, points=points)


@functools.lru_cache(maxsize=None)
def twin_output(shape, kind):
    """OracleEngine.reduced_pieces on the case, computed once for the host test and the GPU test's parity check."""
    from oracle_engine import OracleEngine
    c = case(shape, kind)
    return OracleEngine().reduced_pieces(*c["args"], c["K"], c["node_of"])


@functools.lru_cache(maxsize=None)
def degenerate(shape, seed=0):
    """Pieces whose flag is known from their construction, next to pieces that differ from them in the one thing that makes
    them degenerate.  Duplicates are exact; everything else is Gaussian and well conditioned.
    Node 0 has a PLANTED solution: rows 0, 1, 2 active at their lower bounds with multipliers >= 0.5, every other row inactive
    by >= 0.5, so the recipe Kp = [5, 5, 5, 6, ...] has inside points.  Node 1 is node 0 with row 1 := row 0 (A, B, l, u equal
    bit for bit); node 2 is node 0 with the entries of row 2 of [A B] at most 1e-8 (local_piece drops them); node 3 is node 0
    with row 2 of [A B] exactly zero.
      (a) node 1, Kp: two equal rows active on the same side                                    -> flag bit 0
      (b) node 0, every row code 5, where m > n: more than n active rows                        -> flag bit 0
      (c) node 2, Kp: lambda_2 is held by its own sign row only -- no equality pins it while an alive row holds it, which is
          the header's condition word for word (and what the twin does)                        -> flag bit 0
      (d) node 3, code 8 / code 0 on row 2: nothing holds the column                            -> clear
      (e) node 0, Kp (the neighbour of (a), (b), (c)), and node 0 with code 8 on row 2 (the neighbour of (d): a free multiplier
          on an ordinary row is pinned by a stationarity row)                                   -> clear
    (Flag bit 1, more than n + 2m rows left, cannot happen for node records: of the 2 (n + m) rows, the n rows [I1 0] have
    infinite bounds under code 2 and are never alive, so at most n + 2m are.  Nothing here tries to provoke it.)
    -> dict(rec, args, K, node_of, flags (expected), names, points: {piece: reference points} for the clear pieces that
    reference_points covers)."""
    n, m, p = shape
    assert n >= 3 and m >= 3
    g = np.random.default_rng([seed, 11, n, m, p])
    Q, R, qd, A, B, l, u = [a[0] for a in records(shape, "gauss", seed, nodes=1)]
    w = base_w(p)
    x = 0.5 * g.standard_normal(n)
    lam = np.zeros(m); lam[:3] = 0.5 + np.abs(g.standard_normal(3))
    qd = -(Q @ x + R @ w - A.T @ lam)
    s = A @ x + B @ w
    l = s - 0.5 - np.abs(g.standard_normal(m)); u = s + 0.5 + np.abs(g.standard_normal(m))
    l[:3] = s[:3]
    stack = lambda a: np.stack([a] * 4)
    Q, R, qd, A, B, l, u = [stack(a) for a in (Q, R, qd, A, B, l, u)]
    A[1, 1] = A[1, 0]; B[1, 1] = B[1, 0]; l[1, 1] = l[1, 0]; u[1, 1] = u[1, 0]
    A[2, 2] = 1e-8 * g.uniform(-1.0, 1.0, n); B[2, 2] = 1e-8 * g.uniform(-1.0, 1.0, p)
    A[3, 2] = 0.0; B[3, 2] = 0.0; l[3, 2] = -1.0; u[3, 2] = 1.0
    rec = (Q, R, qd, A, B, l, u)
    Kp = np.full(n + m, 2, np.uint8); Kp[n:] = 6; Kp[n:n + 3] = 5
    with_code = lambda c: np.concatenate([Kp[:n + 2], [c], Kp[n + 3:]]).astype(np.uint8)
    items = [("e: planted recipe", 0, Kp, 0), ("a: equal rows active", 1, Kp, 1), ("c: dropped row active", 2, Kp, 1),
             ("d: free multiplier on a zero row, code 8", 3, with_code(8), 0),
             ("d: free multiplier on a zero row, code 0", 3, with_code(0), 0),
             ("e: free multiplier on an ordinary row", 0, with_code(8), 0)]
    if m > n:
        Kb = Kp.copy(); Kb[n:] = 5
        items.append(("b: more than n active rows", 0, Kb, 1))
    K = np.array([it[2] for it in items], np.uint8); node_of = np.array([it[1] for it in items], np.int32)
    rng = np.random.default_rng([seed, 13, n, m, p])
    points = {t: reference_points(rec, K[t], int(node_of[t]), rng, w) for t in (0, 3, 4)}
    assert len(points[0]["inside"]) >= 4                               # the planted recipe's own piece is populated
    return dict(rec=rec, args=abi(rec), K=K, node_of=node_of, flags=np.array([it[3] for it in items], np.int32),
                names=[it[0] for it in items], points=points)
