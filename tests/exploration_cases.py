"""Shared cases of the multiplier-vertex exploration tests (tests/test_exploration_host.py, tests/test_gpu_exploration.py)."""
import itertools

import numpy as np

import qpn_amd  # noqa: F401
from qpn_amd import level_batch as lb
from qpn_amd.programs import QPNet

INF = np.inf


def counterexample_net(swap=False, **opts):
    """Variables [w1, x, y].  Follower over y: 1/2 (y - w1)^2 s.t. y >= 0, y - x >= 0 (one constraint, two rows); leader over x:
    1/2 (x - 1)^2; edge leader -> follower.  From [-1, 0, 0] the follower sits at y = 0 with both rows active and
    Lambda = {lambda >= 0 : lambda_1 + lambda_2 = 1}; its pieces are {y = x = 0}, {y = 0, x <= 0} and {y = x, x >= 0}."""
    net = QPNet(3)
    A = np.array([[0.0, 0.0, 1.0], [0.0, -1.0, 1.0]])
    if swap:
        A = A[::-1].copy()
    cid = net.add_constraint(A, np.zeros(2), np.full(2, INF))
    fol = net.add_qp(np.array([[1.0, 0, -1], [0, 0, 0], [-1, 0, 1]]), np.zeros(3), [cid], [2])
    Ql = np.zeros((3, 3)); Ql[1, 1] = 1.0
    lead = net.add_qp(Ql, np.array([0.0, -1.0, 0.0]), [], [1])
    net.add_edges([(lead, fol)])
    net.assign_constraint_groups()
    net.set_options(**opts)
    return net, lead, fol


X0 = np.array([-1.0, 0.0, 0.0])


def degenerate_case(rng, n, m, kind="lp"):
    """(Ac [n, m], g [n], cls [m], lam0 [m]): Lambda from a random E = Ad' with g = E lam* for a sparse lam* >= 0, so the
    vertex at lam* is degenerate.  kind 'lp': every row GE; 'mixed': some LE, FREE and ZERO rows, the free columns independent;
    'dependent': duplicated columns (dependent active rows)."""
    E = rng.standard_normal((n, m))
    cls = np.zeros(m, np.uint8)
    if kind == "mixed" and m >= 4:
        cls[rng.permutation(m)[: m // 4]] = lb.MV_LE
        cls[rng.permutation(m)[: max(1, min(n // 2, m // 8))]] = lb.MV_FREE
        cls[rng.permutation(m)[: m // 8]] = lb.MV_ZERO
    if kind == "dependent" and m >= 2:
        k = m // 2
        E[:, k:2 * k] = E[:, :k] * rng.uniform(0.5, 2.0, size=k)
    sig = np.where(cls == lb.MV_LE, -1.0, 1.0)
    lam = np.zeros(m)
    supp = rng.permutation(m)[: max(1, min(n - 1, m) if n > 1 else 1)]
    lam[supp] = rng.uniform(0.5, 2.0, size=supp.size) * sig[supp]
    lam[cls == lb.MV_ZERO] = 0.0
    g = E @ lam
    return E, g, cls, lam


def brute_vertices(E, g, cls, tol=1e-7):
    """Every vertex of Lambda by enumeration over column subsets (small m only), rounded to 5 digits."""
    n, m = E.shape
    sig = np.where(cls == lb.MV_LE, -1.0, 1.0)
    keep = np.nonzero(cls != lb.MV_ZERO)[0]
    free = [j for j in keep if cls[j] == lb.MV_FREE]
    Es = E * sig[None, :]
    r = np.linalg.matrix_rank(Es[:, keep]) if keep.size else 0
    out = set()
    for S in itertools.combinations([j for j in keep if cls[j] != lb.MV_FREE], r - len(free)):
        cols = sorted(free + list(S))
        B = Es[:, cols]
        if np.linalg.matrix_rank(B) < len(cols):
            continue
        mu, *_ = np.linalg.lstsq(B, g, rcond=None)
        if np.max(np.abs(B @ mu - g)) > 1e-7 * max(1.0, np.max(np.abs(g))):
            continue
        if np.any(np.array([mu[k] for k, c in enumerate(cols) if cls[c] != lb.MV_FREE]) < -tol):
            continue
        lam = np.zeros(m); lam[cols] = mu * sig[cols]
        lam[np.abs(lam) < 1e-9] = 0.0
        out.add(tuple(np.round(lam, 5) + 0.0))
    return out
