"""The planted family of the emptiness tests (qpn_exemplar_polys / polyhedra.exemplar_polys_host), shared by the CPU and the GPU
tests: polyhedra with open bounds whose verdict is known by construction and does not depend on which optimal dual a solver
returns."""
from __future__ import annotations

import numpy as np

INF = np.inf
MEMBER, MEMBER_BAND, EMPTY_SLACK, EMPTY_OPEN, ITER_LIMIT, FAILURE = 0, 1, 2, 3, 4, 5
OUTPUTS = ("empty", "how", "eps", "x", "row", "lam", "iters")
KINDS = ("fat", "gap", "thin_open", "thin_else", "thin_closed")
TOL = 1e-4                                       # no eps of the family lies within 1e-5 of +-TOL
HOW = dict(fat=MEMBER, gap=EMPTY_SLACK, thin_open=EMPTY_OPEN, thin_else=MEMBER_BAND, thin_closed=MEMBER_BAND)


def planted(seed, n, d, kind):
    """One polyhedron {x : l <= A x <= u} with open flags, Gaussian rows around a point x0 (s0 = A x0), l = s0 - |N| - 0.05, u = s0 +
    |N| + 0.05, every row two-sided, lower-only or upper-only at random, every flag set with probability 1/2.
      fat          as above: a member, eps <= -0.05
      gap          rows 0 and 1 are a'x <= s0_0 - 1 and a'x >= s0_0 + 1 (n = 1: l = s0 + 1, u = s0 - 1): empty, eps = 1
      thin_open    a random row k has l_k = u_k = s0_k and open_lo_k set: eps = 0 and the dual is unique, lam_k = lam_{n+k} = 1/2: empty
      thin_else    the same row with both of its flags clear, the other rows' flags random: a member in the band
      thin_closed  the same row, every flag clear: a member in the band
    -> (A [n, d], l, u, open_lo, open_hi [n] uint8, empty)."""
    g = np.random.default_rng([seed, n, d, KINDS.index(kind)])
    x0 = g.standard_normal(d)
    A = g.standard_normal((n, d))
    s0 = A @ x0
    l = s0 - np.abs(g.standard_normal(n)) - 0.05; u = s0 + np.abs(g.standard_normal(n)) + 0.05
    sided = g.integers(0, 3, n)
    l = np.where(sided == 2, -INF, l); u = np.where(sided == 1, INF, u)
    open_lo = (g.random(n) < 0.5).astype(np.uint8); open_hi = (g.random(n) < 0.5).astype(np.uint8)
    k = int(g.integers(0, n))
    if kind == "gap":
        if n == 1:
            l[0], u[0] = s0[0] + 1.0, s0[0] - 1.0
        else:
            A[1] = A[0]
            l[0], u[0] = -INF, s0[0] - 1.0
            l[1], u[1] = s0[0] + 1.0, INF
    elif kind != "fat":
        l[k] = u[k] = s0[k]
        if kind == "thin_open":
            open_lo[k] = 1
        elif kind == "thin_else":
            open_lo[k] = open_hi[k] = 0
        else:
            open_lo[:] = 0; open_hi[:] = 0
    return A, l, u, open_lo, open_hi, kind in ("gap", "thin_open")


def family_batch(shape, count, first=0):
    """`count` polyhedra of one shape, the five kinds in turn (polyhedron t: seed first + t, kind t % 5).
    -> (A [count, n, d], l, u, open_lo, open_hi [count, n], empty [count] bool, how [count])."""
    n, d = shape
    cases = [planted(first + t, n, d, KINDS[t % 5]) for t in range(count)]
    stack = lambda i: np.stack([c[i] for c in cases])
    return stack(0), stack(1), stack(2), stack(3), stack(4), np.array([c[5] for c in cases]), np.array([HOW[KINDS[t % 5]] for t in range(count)])


def family_polys(shapes=((1, 1), (3, 2), (8, 4)), count=15):
    """The family as Poly objects (rows as given: no normalisation, so the plant's flags stay on their sides).  -> (polys, empty)."""
    from qpn_amd.programs import Poly
    polys, empty = [], []
    for shape in shapes:
        A, l, u, ol, oh, e, _ = family_batch(shape, count)
        polys += [Poly(A[t], l[t], u[t], normalise=False, open_lo=ol[t].astype(bool), open_hi=oh[t].astype(bool)) for t in range(count)]
        empty += list(e)
    return polys, np.array(empty)


def same_bits(got, want, what):
    for k in OUTPUTS:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        w = np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        diff = np.nonzero(g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1))[0]
        assert diff.size == 0, (what, k, diff[:8], g[diff[:2]], w[diff[:2]])
