"""The subset cases of tests/test_subset_pairs_host.py and tests/test_gpu_subset_pairs.py: the seeded family of pairs (P1, P2) and
its batches.  The outcome codes are those of include/qpn_hip.h (QPN_SUBSET_*)."""
import numpy as np

HOLDS, BY_POINT, BY_OPTIMUM, UNBOUNDED, ITER_LIMIT, FAILURE, EMPTY = 0, 1, 2, 3, 4, 5, 6
SHAPES = [(1, 1, 1), (3, 2, 2), (5, 4, 2), (12, 9, 6), (16, 16, 8), (40, 33, 24)]
OUTPUTS = ("sub", "how", "bound", "val", "lps", "iters")


def family_pair(r1, r2, d, seed):
    """-> (A1 [r1, d], l1, u1, A2 [r2, d], l2, u2); the kind is seed % 6.  P1: Gaussian rows two-sided around a point x0.  P2: even
    rows are rows of P1 copied exactly with their bounds widened by 0.25, odd rows Gaussian and far out; a random third of the rows
    lose their lower bound, a third their upper one.  Kind 1: a shared row of P2 cuts P1 through its middle; 2: a fresh row of P2
    cuts just above x0; 3: P1 open below on every row; 4: a contradictory pair of rows in P1; 0, 5: unchanged."""
    kind = seed % 6
    rng = np.random.default_rng(7000 + seed)
    A1 = rng.standard_normal((r1, d))
    x0 = rng.standard_normal(d)
    s0 = A1 @ x0
    l1 = s0 - np.abs(rng.standard_normal(r1)) - 0.05; u1 = s0 + np.abs(rng.standard_normal(r1)) + 0.05
    A2 = np.empty((r2, d)); l2 = np.empty(r2); u2 = np.empty(r2)
    shared = []
    for i in range(r2):
        if i % 2 == 0:
            k = int(rng.integers(0, r1))
            A2[i] = A1[k]; l2[i] = l1[k] - 0.25; u2[i] = u1[k] + 0.25
            shared.append((i, k))
        else:
            A2[i] = rng.standard_normal(d)
            c = A2[i] @ x0
            far = 8.0 * np.sqrt(d) + 4.0
            l2[i] = c - far; u2[i] = c + far
    side = rng.integers(0, 3, r2)                            # 0 both, 1 no lower bound, 2 no upper bound
    l2 = np.where(side == 1, -np.inf, l2); u2 = np.where(side == 2, np.inf, u2)
    if kind == 1:
        i, k = shared[int(rng.integers(0, len(shared)))]
        l2[i] = -np.inf; u2[i] = 0.5 * (l1[k] + u1[k])
    if kind == 2:
        i = min(r2 - 1, 1)
        A2[i] = rng.standard_normal(d)
        l2[i] = A2[i] @ x0 + 0.01; u2[i] = np.inf
    if kind == 3:
        l1 = np.full(r1, -np.inf)
    if kind == 4 and r1 >= 2:                                # a'x <= s0 - 1 and a'x >= s0 + 1
        A1[1] = A1[0]; l1[0], u1[0] = -np.inf, s0[0] - 1.0; l1[1], u1[1] = s0[0] + 1.0, np.inf
    return A1, l1, u1, A2, l2, u2


def family_batch(shape, seeds):
    """The family's pairs of one shape as a batch: first piece k and second piece k are those of seeds[k].
    -> (A1 [B, r1, d], l1, u1 [B, r1], A2 [B, r2, d], l2, u2 [B, r2])."""
    cases = [family_pair(*shape, s) for s in seeds]
    return tuple(np.stack([c[k] for c in cases]) for k in range(6))


def same_bits(got, want, what):
    for k in OUTPUTS:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        w = np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype)
        diff = np.nonzero(g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1))[0]
        assert diff.size == 0, (what, k, diff[:8], g[diff[:2]], w[diff[:2]])
