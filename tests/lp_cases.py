"""The LP cases of tests/test_lp_host.py and tests/test_gpu_lp.py: the seeded family and the certificate checks, in plain numpy on
the unscaled data.  The conditions are the ones include/qpn_hip.h states for qpn_solve_lps at check_tol = 1e-6."""
import numpy as np

OPTIMAL, INFEASIBLE, UNBOUNDED, ITER_LIMIT, FAILURE = 1, 2, 3, 4, 5
CT = 1e-6


def family_case(seed, rmax=16, dmax=8, shape=None):
    """-> (A [r, d], l, u [r], c [d], (row, sign) or None).  Gaussian rows, one fifth rounded to integers, one seventh with a row
    equal to the sum of two others; every row free, one-sided or two-sided at random; one quarter with a contradictory pair of
    rows; one third with a row of the polyhedron (times +-1) as the objective.  shape = (r, d) fixes the size."""
    rng = np.random.default_rng(1000 + seed)
    r = int(rng.integers(1, rmax + 1)); d = int(rng.integers(1, dmax + 1))
    if shape is not None:
        r, d = shape
    A = rng.standard_normal((r, d))
    if seed % 5 == 0:
        A = np.round(2.0 * A)
    if seed % 7 == 3 and r >= 3:
        A[2] = A[0] + A[1]
    x0 = rng.standard_normal(d)
    s0 = A @ x0
    l = s0 - np.abs(rng.standard_normal(r)); u = s0 + np.abs(rng.standard_normal(r))
    kind = rng.integers(0, 4, r)                            # 0 two-sided, 1 lower only, 2 upper only, 3 free
    l = np.where((kind == 2) | (kind == 3), -np.inf, l); u = np.where((kind == 1) | (kind == 3), np.inf, u)
    if seed % 4 == 1 and r >= 2:                            # a'x <= s0 - 1 and a'x >= s0 + 1
        A[1] = A[0]; l[0], u[0] = -np.inf, s0[0] - 1.0; l[1], u[1] = s0[0] + 1.0, np.inf
    if seed % 3 == 2:
        row = (int(rng.integers(0, r)), int(rng.choice([-1, 1])))
        return A, l, u, row[1] * A[row[0]], row
    return A, l, u, rng.standard_normal(d), None


def check_certificates(A, l, u, c, got):
    """What a job's outputs claim, checked on the unscaled data.  got: dict(status, x, obj, lam, ray, iters) of ONE job."""
    st = int(got["status"]); x, lam, ray = got["x"], got["lam"], got["ray"]
    with np.errstate(invalid="ignore"):
        s = A @ x
        tl = CT * np.maximum(1.0, np.abs(l)); tu = CT * np.maximum(1.0, np.abs(u))
        if st in (OPTIMAL, UNBOUNDED):
            assert np.all(s >= l - tl) and np.all(s <= u + tu)
            assert abs(got["obj"] - c @ x) <= 1e-12 * max(1.0, abs(c @ x))
        if st == OPTIMAL:
            assert np.all(np.abs(c - A.T @ lam) <= CT * np.maximum(1.0, np.abs(c)))
            assert np.all(np.abs(s - l)[lam > CT] <= tl[lam > CT])            # + at the lower bound
            assert np.all(np.abs(s - u)[lam < -CT] <= tu[lam < -CT])          # - at the upper bound
            assert not ray.any()
        elif st == UNBOUNDED:
            ar = A @ ray
            tr = CT * max(1.0, np.max(np.abs(ray))) * np.max(np.abs(A), axis=1)
            assert c @ ray < 0.0
            assert np.all(ar[np.isfinite(l)] >= -tr[np.isfinite(l)]) and np.all(ar[np.isfinite(u)] <= tr[np.isfinite(u)])
            assert not lam.any()
        elif st == INFEASIBLE:
            assert np.all(np.abs(A.T @ lam) <= CT * max(1.0, np.max(np.abs(lam))))
            assert np.all(np.isfinite(u[lam > 0.0])) and np.all(np.isfinite(l[lam < 0.0]))
            # negative by more than the bounds relaxed by the tolerance primal feasibility is judged at account for: a residual of
            # A'y that is tolerated at CT * |y| makes a sum nearer to zero prove nothing
            slack = np.sum(lam[lam > 0.0] * tu[lam > 0.0]) - np.sum(lam[lam < 0.0] * tl[lam < 0.0])
            assert np.sum(lam[lam > 0.0] * u[lam > 0.0]) + np.sum(lam[lam < 0.0] * l[lam < 0.0]) < -slack
            assert not ray.any()
        else:
            assert not lam.any() and not ray.any()


def family_batch(shape, seeds):
    """The family's cases of one shape as a batch over shared polyhedra: polyhedron k is the case of seeds[k]; its jobs are the
    case's own objective and, in a second batch, every (row, sign) of it.
    -> (A [polys, r, d], l, u [polys, r], cost [polys, d], poly_of_rows, obj_row, obj_sign)."""
    cases = [family_case(s, shape=shape) for s in seeds]
    r, d = shape
    A = np.stack([c[0] for c in cases]); l = np.stack([c[1] for c in cases]); u = np.stack([c[2] for c in cases])
    cost = np.stack([c[3] for c in cases])
    poly_of = np.repeat(np.arange(len(seeds)), 2 * r).astype(np.int32)
    obj_row = np.tile(np.repeat(np.arange(r), 2), len(seeds)).astype(np.int32)
    obj_sign = np.tile([1, -1], r * len(seeds)).astype(np.int32)
    return A, l, u, cost, poly_of, obj_row, obj_sign


def bounded_batch(seed, polys, r, d):
    """Gaussian polytopes around a point, every row two-sided (row objectives are bounded on them).  -> (A, l, u)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((polys, r, d))
    s0 = np.einsum("brd,bd->br", A, rng.standard_normal((polys, d)))
    return A, s0 - np.abs(rng.standard_normal((polys, r))) - 0.05, s0 + np.abs(rng.standard_normal((polys, r))) + 0.05
