"""Degenerate polyhedra with planted answers for the LP entries (tests/test_lp_degenerate_host.py, tests/test_gpu_lp_degenerate.py):
many rows through one vertex, a polyhedron that is a single point, a cone cut off beyond its degenerate apex, the
assignment polytope, and rows repeated at scales from 2**-20 to 2**20.  Plain numpy.  The data of cone / pinned / capped are
quarter-integers of moderate size, so every product and sum the generators assert is exact in floating point: the planted facts are
asserted without a tolerance."""
import numpy as np

INF = np.inf
NONFINITE_KINDS = ("A", "l", "u", "c", "l=+inf", "u=-inf")


def cone(seed, r, d, q=4):
    """r rows through the point x0, c inside their normal cone.  -> (A [r, d], l, u [r], c [d], x0 [d]).
    Planted: min c'x is OPTIMAL at x0 with objective c @ x0 (for every x of the cone c'x - c'x0 = sum lam_i (a_i'x - l_i) >= 0)."""
    g = np.random.default_rng(seed)
    A = np.round(q * g.standard_normal((r, d))) / q
    A[~A.any(axis=1)] = 1.0
    x0 = np.round(q * g.standard_normal(d)) / q
    l = A @ x0
    u = np.full(r, INF)
    lam = g.integers(1, 5, r).astype(np.float64)
    c = A.T @ lam
    # exact: every entry is a multiple of 1 / q**2 far below 2**53 / q**2, in whatever order it is summed
    assert np.all(np.round(A * q) == A * q) and np.all(np.round(l * q * q) == l * q * q) and np.all(np.round(c * q) == c * q)
    assert np.all(A @ x0 >= l) and np.all(A @ x0 <= u) and np.all(A @ x0 == l)
    assert np.all(A.T @ lam == c) and (c @ x0) * q * q == np.round((c @ x0) * q * q) and c @ x0 == lam @ l
    return A, l, u, c, x0


def pinned(seed, r, d):
    """cone plus the row c'x <= c @ x0: the set is {x0}, r + 1 rows.  -> (A [r + 1, d], l, u [r + 1], x0).
    (c'x - c'x0 = sum lam_i (a_i'x - l_i) with every lam_i >= 1, so c'x <= c'x0 forces every row to its bound; the rows span R^d
    whenever they have rank d, which the generator asserts.)
    Planted: never INFEASIBLE / EMPTY; every (row, sign) LP is OPTIMAL with objective sign * a_i @ x0; implicit_bounds is OK with eq
    all ones and vals = A @ x0."""
    A, l, u, c, x0 = cone(seed, r, d)
    A = np.vstack([A, c]); l = np.append(l, -INF); u = np.append(u, c @ x0)
    assert np.all(A @ x0 >= l) and np.all(A @ x0 <= u)
    assert np.linalg.matrix_rank(A[:r]) == d
    return A, l, u, x0


def capped(seed, r, d):
    """cone plus the row c'x <= c @ x0 + 1: the cone cut off beyond its degenerate apex x0, a polytope (c'x - c'x0 = sum lam_i
    (a_i'x - l_i) with every lam_i >= 1 bounds every row by l_i + 1; the rows have rank d).  Whether it has an interior depends on
    the draw: r Gaussian half-spaces through one point seldom share more than the point when r is several times d.
    -> (A, l, u [r + 1], x0).
    Planted: with all_extremes the result is OK, lo[i] = l[i] on the r cone rows (reached at x0) and lo[r] = c @ x0.  The upper
    extremes have no planted value: an independent LP solver on the same data, which is well scaled, gives them."""
    A, l, u, c, x0 = cone(seed, r, d)
    A = np.vstack([A, c]); l = np.append(l, -INF); u = np.append(u, c @ x0 + 1.0)
    assert np.all(A @ x0 >= l) and np.all(A @ x0 <= u)
    assert np.linalg.matrix_rank(A[:r]) == d
    return A, l, u, x0


def relaxed(l, u, by=1e-3):
    """Every finite bound moved out by `by`."""
    return l - by, u + by                                  # (-inf - by = -inf)


def box(lo, hi):
    """-> (I, lo, hi): the box as a polyhedron."""
    lo = np.asarray(lo, dtype=np.float64)
    return np.eye(len(lo)), lo, np.asarray(hi, dtype=np.float64)


def assignment(seed, k):
    """The k x k assignment polytope, d = k * k: rows I with [0, inf), then the k row sums and the k column sums fixed at 1; an
    integer cost in 1..19.  -> (A [k k + 2 k, k k], l, u, c).
    Planted: the optimum is scipy.optimize.linear_sum_assignment's; all_extremes finds exactly the 2 k sum rows EXPLICIT, and every
    x row has lo = 0, hi = 1 (every entry is 0 in one permutation matrix and 1 in another)."""
    g = np.random.default_rng(seed)
    d = k * k
    S = np.zeros((2 * k, d))
    for i in range(k):
        S[i, i * k:(i + 1) * k] = 1.0                      # row i of the matrix
        S[k + i, i::k] = 1.0                               # column i
    A = np.vstack([np.eye(d), S])
    l = np.concatenate([np.zeros(d), np.ones(2 * k)]); u = np.concatenate([np.full(d, INF), np.ones(2 * k)])
    c = g.integers(1, 20, d).astype(np.float64)
    x = np.eye(k).ravel()
    assert np.all(A @ x >= l) and np.all(A @ x <= u)
    return A, l, u, c


def scaled_copies(seed, r, d, row_scales):
    """A Gaussian base polytope of k = max(d + 1, r // 3) two-sided rows around a point, then r - k copies of random base rows, each
    times +-2**e, e in -20..20 (the bounds swapped when the sign is negative: the same half-spaces, exactly, since a power of two
    scales without rounding); with row_scales every row of the result is then multiplied by 10**e, e in -4..3.
    -> (A [r, d], l, u [r], c [d], (Ab, lb, ub): the base polytope).
    The set is the base polytope's: the reference is an LP solver ON THE BASE, not on the scaled data.  Without row_scales the copies
    are exact ties after the row scaling of the LP entries: the tie-breaking case."""
    g = np.random.default_rng(seed)
    k = max(d + 1, r // 3)
    Ab = g.standard_normal((k, d))
    s0 = Ab @ g.standard_normal(d)
    lb = s0 - np.abs(g.standard_normal(k)) - 0.05; ub = s0 + np.abs(g.standard_normal(k)) + 0.05
    src = g.integers(0, k, r - k)
    f = np.where(g.random(r - k) < 0.5, -1.0, 1.0) * 2.0 ** g.integers(-20, 21, r - k)
    A = np.vstack([Ab, Ab[src] * f[:, None]])
    l = np.concatenate([lb, np.where(f > 0, lb[src] * f, ub[src] * f)])
    u = np.concatenate([ub, np.where(f > 0, ub[src] * f, lb[src] * f)])
    assert np.all(l < u)
    if row_scales:
        m = 10.0 ** g.integers(-4, 4, r)
        A = A * m[:, None]; l = l * m; u = u * m
    c = g.standard_normal(d)
    return A, l, u, c, (Ab, lb, ub)


def with_nonfinite(case, what):
    """`case` = (A, l, u, c, ...) with one non-finite value planted: a NaN in A[5, 2], l[5], u[5] or c[1], or an infinity on the wrong
    side of a bound of row 5 (the tests use cone(3, 12, 4)).  -> (A, l, u, c), copies."""
    A, l, u, c = (np.array(a, dtype=np.float64) for a in case[:4])
    if what == "A":
        A[5, 2] = np.nan
    elif what == "l":
        l[5] = np.nan
    elif what == "u":
        u[5] = np.nan
    elif what == "c":
        c[1] = np.nan
    elif what == "l=+inf":
        l[5] = INF
    elif what == "u=-inf":
        u[5] = -INF
    else:
        raise ValueError(what)
    return A, l, u, c


def row_jobs(r, polys=1):
    """Every (row, sign) of `polys` polyhedra of r rows.  -> (poly_of, obj_row, obj_sign) int32."""
    poly_of = np.repeat(np.arange(polys), 2 * r).astype(np.int32)
    obj_row = np.tile(np.repeat(np.arange(r), 2), polys).astype(np.int32)
    obj_sign = np.tile([1, -1], r * polys).astype(np.int32)
    return poly_of, obj_row, obj_sign
