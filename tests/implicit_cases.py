"""The cases of tests/test_implicit_bounds_host.py and tests/test_gpu_implicit_bounds.py: the seeded family of tests/lp_cases.py with
a planted implicit equality, the polytopes of the class boundaries, and the bit comparison of two answers.  The codes are those of
include/qpn_hip.h (QPN_IB_*, QPN_IB_HOW_*)."""
import numpy as np

import lp_cases

OK, EMPTY, ITER_LIMIT, FAILURE = 0, 1, 2, 3
UNDECIDED, EXPLICIT, IMPLICIT, BY_POINTS, BY_EXTREMES, UNBOUNDED = 0, 1, 2, 3, 4, 5
OUTPUTS = ("status", "fail_row", "eq", "vals", "how", "lo", "hi", "lps", "iters")
PINNED = (np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), np.array([1.0, -np.inf, 0.0]), np.array([np.inf, 1.0, np.inf]))


def family_case(seed, shape):
    """-> (A [r, d], l, u [r]): lp_cases.family_case(seed, shape=shape); on even seeds (never the contradictory ones, seed % 4 == 1)
    with r >= 4 the last two rows are replaced by a'x <= b and -2 a'x <= -2 b through the case's own feasible point x0: one
    implicit equality, both of whose rows are to be found."""
    A, l, u, _, _ = lp_cases.family_case(seed, shape=shape)
    r, d = shape
    if seed % 2 == 0 and seed % 4 != 1 and r >= 4:
        rng = np.random.default_rng(1000 + seed)             # (lp_cases.family_case's draws up to its point x0)
        rng.integers(1, 17); rng.integers(1, 9); rng.standard_normal((r, d))
        x0 = rng.standard_normal(d)
        with np.errstate(invalid="ignore"):
            assert np.all(A @ x0 >= l) and np.all(A @ x0 <= u)
        a = np.random.default_rng(5000 + seed).standard_normal(d)
        b = float(a @ x0)
        A[r - 2] = a; l[r - 2] = -np.inf; u[r - 2] = b
        A[r - 1] = -2.0 * a; l[r - 1] = -np.inf; u[r - 1] = -2.0 * b
    return A, l, u


def family_batch(shape, seeds):
    """-> (A [polys, r, d], l, u [polys, r]): polyhedron k is the case of seeds[k]."""
    cases = [family_case(s, shape) for s in seeds]
    return tuple(np.stack([c[k] for c in cases]) for k in range(3))


def boundary_batch(seed, r, d):
    """Three polytopes of lp_cases.bounded_batch(seed, 3, r, d); in each, row 0 alone reads x_0 and is open below (its minimum
    is unbounded), and rows 1, 2 are an opposite pair a'x <= b, -a'x <= -b through the polytope's centre (an implicit equality)."""
    A, l, u = lp_cases.bounded_batch(seed, 3, r, d)
    for b in range(3):
        centre = np.linalg.lstsq(A[b], 0.5 * (l[b] + u[b]), rcond=None)[0]
        A[b, 1:, 0] = 0.0
        s = A[b] @ centre
        l[b] = s - 1.0 - 0.1 * np.arange(r) / r; u[b] = s + 1.0 + 0.1 * np.arange(r) / r
        l[b, 0] = -np.inf
        A[b, 2] = -A[b, 1]
        l[b, 1] = -np.inf; u[b, 1] = s[1]
        l[b, 2] = -np.inf; u[b, 2] = -s[1]
    return A, l, u


def same_bits(got, want, what):
    for k in OUTPUTS:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        w = np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        diff = np.nonzero(g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1))[0]
        assert diff.size == 0, (what, k, diff[:8], g[diff[:2]], w[diff[:2]])
