"""Seeded node records with a PLANTED, exactly known solution, and the route matrix of qpn_solve_nodes* they are run through.

make_node plants z* = [x*; lam*]: k active rows (up to three quarters of min(n, m); kfull: all of them) with random sides and
|lam*_i| in [0.5, 1.5], inactive rows at least 0.2 inside
their bounds (mixed bound kinds: an infinite bound only on a side that is not active), qd := A_act' lam* - Qd x* - R w formed in
longdouble and rounded once, active bounds := fl(Ad x* + B w).  The exact solution of the ROUNDED data is then within
cond * eps of the plant; tests/solve_ref.py computes it and proves it by its certificate.  replant() plants a second solution on
the same Qd, R, Ad, B (what qpn_nodes_update of qd, l, u leaves of a crash cache).

Families: k40 (the suite's spectrum, Q = G'G/n + 0.1 I), k1e4 / k1e6 (rotated geometric spectrum 1 .. 1/kappa, bitwise
symmetric), axis (diagonal Q, spectrum 1 .. 1e-5 permuted: diagonals below the fused kernels' decline threshold), skew (k40 +
0.5 (S - S')/sqrt(n)), nearsym (k40 + 1e-7 (S - S')/sqrt(n): reading the mirrored tile is wrong by ~1e-7), weak (two inactive
rows exactly on a bound, zero multiplier), k0 / kfull (no / min(n, m) active rows), rowscale (row norms log-uniform in
[1/30, 30]; multipliers and slacks scale with them).
"""
from __future__ import annotations

import numpy as np

import solve_ref as SR

LD = np.longdouble
FAMILIES = ("k40", "k1e4", "k1e6", "axis", "skew", "nearsym", "weak", "k0", "kfull", "rowscale")
SYMMETRIC = ("k40", "k1e4", "k1e6", "axis", "weak", "k0", "kfull", "rowscale")
RESIDENT = 16 * 256                       # kResidentMI355X (csrc/qpn_internal.h): a reuse sweep beyond it is a mixed launch


def _ld(a):
    return np.asarray(a, dtype=LD)


def _hessian(rng, n, family):
    if family in ("k1e4", "k1e6"):
        V, _ = np.linalg.qr(rng.standard_normal((n, n)))
        Q = (V * np.geomspace(1.0, 1.0 / float(family[1:]), n)) @ V.T
        return 0.5 * (Q + Q.T)                            # (a + b == b + a: bitwise symmetric)
    if family == "axis":
        return np.diag(rng.permutation(np.geomspace(1.0, 1e-5, n)))
    G = rng.standard_normal((n, n))
    Q = G.T @ G / n + 0.1 * np.eye(n)
    if family in ("skew", "nearsym"):
        S = rng.standard_normal((n, n))
        Q = Q + (0.5 if family == "skew" else 1e-7) * (S - S.T) / np.sqrt(n)
    return Q


def replant(rng, node):
    """A (new) planted solution on the node's Qd, R, Ad, B, w: sets qd, l, u, side (+1 at l, -1 at u, 0 inactive), plant."""
    Q, R, _, A, B, _, _ = node["rec"]
    w, family = node["w"], node["family"]
    n, m = Q.shape[0], A.shape[0]
    scale = node["row_scale"]
    # (up to three quarters of min(n, m) active rows: a nearly square A_act is the kfull family's subject, and its condition
    #  number would otherwise set the error of whichever family happens to draw it)
    k = {"k0": 0, "kfull": min(n, m)}.get(family, int(rng.integers(0, min(max(1, 3 * min(n, m) // 4), m) + 1)))
    if family == "weak":
        k = min(k, max(min(n, m) - 2, 0))                 # (the two weakly active rows are on a bound too: at most n such rows)
    rows = np.sort(rng.permutation(m)[:k])
    side = np.zeros(m, dtype=np.int8)
    side[rows] = rng.choice([-1, 1], size=k)
    x = rng.standard_normal(n)
    lam = np.zeros(m)
    lam[rows] = side[rows] * rng.uniform(0.5, 1.5, k) / scale[rows]
    a = _ld(A) @ _ld(x) + (_ld(B) @ _ld(w) if w.size else LD(0))
    qd = np.asarray(_ld(A).T @ _ld(lam) - _ld(Q) @ _ld(x) - (_ld(R) @ _ld(w) if w.size else LD(0)), dtype=np.float64)
    a64 = np.asarray(a, dtype=np.float64)                 # fl(Ad x* + B w): the active bounds
    l = a64 - rng.uniform(0.2, 1.5, m) * scale
    u = a64 + rng.uniform(0.2, 1.5, m) * scale
    kind = rng.random(m)
    l[(kind < 0.25) & (side <= 0)] = -np.inf              # one-sided rows; an active side stays finite
    u[(kind > 0.75) & (side >= 0)] = np.inf
    l[side > 0] = a64[side > 0]
    u[side < 0] = a64[side < 0]
    weak = np.zeros(m, dtype=bool)
    if family == "weak":
        for i, up in zip(np.flatnonzero(side == 0)[:2], (False, True)):
            weak[i] = True
            if up:
                u[i] = a64[i]
            else:
                l[i] = a64[i]
    node.update(rec=(Q, R, qd, A, B, l, u), side=side, plant=np.concatenate([x, lam]), weak=weak)
    return node


def make_node(rng, n, m, family, p=3, w=None):
    """One planted node: dict(rec=(Q, R, qd, A, B, l, u) in math layout, w (drawn here unless given: a batch shares one), side,
    plant, weak, family, row_scale)."""
    assert family in FAMILIES
    Q = _hessian(rng, n, family)
    scale = np.exp(rng.uniform(-np.log(30.0), np.log(30.0), m)) if family == "rowscale" else np.ones(m)
    A = rng.standard_normal((m, n)) / np.sqrt(n)
    A *= (scale / np.maximum(np.linalg.norm(A, axis=1), 1e-300))[:, None] if family == "rowscale" else 1.0
    B = 0.3 * rng.standard_normal((m, p)) * scale[:, None]
    R = 0.1 * rng.standard_normal((n, p))
    node = dict(rec=(Q, R, None, A, B, None, None), w=rng.standard_normal(p) if w is None else w, family=family, row_scale=scale)
    return replant(rng, node)


def row_norm(node):
    """|Ad_i| per row for the rowscale family's error measure, None elsewhere."""
    return np.linalg.norm(node["rec"][3], axis=1) if node["family"] == "rowscale" else None


def stack(nodes):
    """Nodes of one shape -> (Q, R, qd, A, B, l, u) stacked (math layout)."""
    return tuple(np.stack([c["rec"][j] for c in nodes]) for j in range(7))


def truth(node):
    """(z*, info) of solve_ref.solve_reference from the plant's active set; computed once per node and kept with it."""
    if "_truth" not in node:
        node["_truth"] = SR.solve_reference(*node["rec"], node["w"], node["side"])
    return node["_truth"]


# ---- the route matrix of solve_nodes_launch (csrc/qpn_capi_nodes.hip) / qpn_solve_avi_batch (csrc/qpn_capi.hip) -------------
# cell -> shapes (n, m, p, nodes per family).  The smallest shapes at which each kernel's tiling can go wrong: the class's
# corners, ragged sides, one side tiny; p = 0 once per fused class.
CELLS = {
    "f32_call":       [(32, 32, 3, 3), (1, 1, 3, 3), (5, 7, 0, 3), (17, 32, 3, 3), (32, 9, 3, 3)],
    "f32_handle_sym": [(32, 32, 3, 4)],
    "f32_handle_gen": [(32, 32, 3, 4)],
    "f32_mixed":      [(32, 32, 3, 8)],
    "s48":            [(33, 33, 3, 3), (48, 40, 3, 3), (40, 3, 0, 3), (9, 48, 3, 3)],
    "wg":             [(49, 49, 3, 3), (64, 64, 3, 3), (64, 12, 0, 3), (20, 57, 3, 3)],
    "wg2":            [(65, 65, 3, 3), (128, 100, 3, 3), (30, 128, 3, 3), (128, 7, 0, 3)],
    "big2":           [(129, 16, 3, 3), (130, 96, 3, 3), (72, 130, 3, 3), (256, 256, 3, 0)],
    "general":        [(20, 0, 3, 3), (40, 130, 3, 3), (260, 10, 3, 3)],
    "explicit_M":     [(32, 32, 3, 3), (100, 128, 3, 3)],
}
ROUTE = dict(f32_call="fused32", f32_handle_sym="fused32", f32_handle_gen="fused32", f32_mixed="fused32", s48="s48", wg="wg",
             wg2="wg2", big2="big2", general="general")
BIG_FAMILIES = ("k40", "k1e4", "axis")                    # the (256, 256) shape of big2: three nodes, one of a family


def cell_families(cell, n, m):
    """The families a cell stacks.  f32_handle_sym / f32_mixed: the symmetric ones (one asymmetric record switches the whole
    handle to the general variants -- f32_handle_gen's subject).  The weak family needs two inactive rows."""
    if cell == "f32_handle_gen":
        return ("skew", "nearsym")
    if (n, m) == (256, 256):
        return BIG_FAMILIES
    fams = SYMMETRIC if cell in ("f32_handle_sym", "f32_mixed") else FAMILIES
    return tuple(f for f in fams if not (f == "weak" and min(n, m) < 3))


def route_of(n, m, mid_route=1, max_pivots=0):
    """node_route (csrc/qpn_capi_nodes.hip) and the shape predicates of the fused kernels, restated."""
    if n <= 32 and 1 <= m <= 32:
        return "fused32"
    budget = max_pivots <= 0 or max_pivots - n >= 1
    wg = (n > 32 or m > 32) and 1 <= n <= 64 and 1 <= m <= 64
    wg2 = (n > 64 or m > 64) and 1 <= n <= 128 and 1 <= m <= 128
    if budget and mid_route == 1 and (wg or wg2):
        return "wg2" if wg2 else ("s48" if n <= 48 and m <= 48 else "wg")
    if budget and 64 < n <= 256 and 1 <= m <= 256:
        return "big2"
    return "general"


_CACHE = {}


def cell_cases(cell, seed=11):
    """[(n, m, p, [nodes])] of one cell, every family stacked per shape (built once per process: the tests share them and leave
    them unchanged)."""
    if (cell, seed) not in _CACHE:
        out = []
        for n, m, p, per in CELLS[cell]:
            rng = np.random.default_rng([seed, sum(map(ord, cell)), n, m])
            fams = cell_families(cell, n, m)
            w = rng.standard_normal(p)                    # one parameter vector per batch (stride_w = 0)
            nodes = [make_node(rng, n, m, f, p, w) for f in fams for _ in range(per or 1)]
            out.append((n, m, p, nodes))
        _CACHE[cell, seed] = out
    return _CACHE[cell, seed]


def second_plants(cell, seed=11):
    """The cell's first shape again with a SECOND planted solution on the same Qd, R, Ad, B, w (new x*, new active set)."""
    if (cell, seed, 2) not in _CACHE:
        n, m, p, nodes = cell_cases(cell, seed)[0]
        rng = np.random.default_rng([seed, 2, sum(map(ord, cell))])
        _CACHE[cell, seed, 2] = [replant(rng, {k: v for k, v in c.items() if k != "_truth"}) for c in nodes]
    return _CACHE[cell, seed, 2]


def per_node_params(cell, nodes, seed=11):
    """Parameters of a sweep with one w per node (stride_w != 0): the batch's w moved by 0.05 N(0, 1) per node -- B dw is well
    inside the 0.2 slack of the inactive rows, so every node stays feasible (the rows of a node with m >> n leave little room)."""
    w = nodes[0]["w"]
    n, m = nodes[0]["rec"][3].shape[::-1]
    rng = np.random.default_rng([seed, 3, sum(map(ord, cell)), n, m])
    return w[None, :] + 0.05 * rng.standard_normal((len(nodes), w.size))


def oracle_solve(oracle, nodes, w, max_pivots=0):
    """The CPU oracle (oracle/binding.py, handed in: this module does not import it) on the nodes' reduced KKT blocks; w (p,) or
    (batch, p)."""
    import problems as P
    M, q, lo, hi, kind = P.reduced_blocks(*stack(nodes), w)
    o = oracle.default_opts()
    o.max_pivots = max_pivots
    return oracle.solve_avi_batch(M, q, lo, hi, kind=kind, opts=o)


def truth_from_solution(node, w, z):
    """(z*, info) for other parameters than the plant's, from the active set some solver's answer claims (the signs of its
    multipliers): the certificate inside solve_reference is the proof, wherever the hint came from."""
    n = node["rec"][0].shape[0]
    zt, info = SR.solve_reference(*node["rec"], w, np.sign(z[n:]).astype(np.int8))
    info["w"] = w
    return zt, info


def check_against_truth(nodes, truths, res, where, tally, e_ref=None, factor=None, masks=True):
    """One solver's outputs (dict of arrays: z, status, active) on `nodes` against their truths -> list of failure messages.
    tally[family] collects [worst error, count]; with e_ref (family -> the oracle's worst error) the accuracy bar is applied,
    with `factor` (family -> factor) overriding solve_ref.FACTOR for single families."""
    fails = []
    z, st, act = np.asarray(res["z"]), np.asarray(res["status"]), np.asarray(res["active"])
    for i, (c, (zt, info)) in enumerate(zip(nodes, truths)):
        fam = c["family"]
        n = c["rec"][0].shape[0]
        tag = f"{where} [{i}] {fam} n={n} m={c['rec'][3].shape[0]} cond={info['cond']:.1e}"
        if not info["ok"]:
            fails.append(f"{tag}: no certified truth ({info['why']})")
            continue
        if st[i] != 1:
            fails.append(f"{tag}: status {st[i]}")
            continue
        e = SR.node_error(z[i], zt, n, row_norm(c))
        t = tally.setdefault(fam, [0.0, 0])
        t[0] = max(t[0], e); t[1] += 1
        if e_ref is not None:
            bar = SR.accuracy_bar(e_ref[fam], (factor or {}).get(fam, SR.FACTOR))
            if not e <= bar:
                fails.append(f"{tag}: error {e:.3e} > bar {bar:.3e} (oracle {e_ref[fam]:.3e})")
        if masks and fam != "rowscale":
            w = info.get("w", c["w"])
            if not SR.mask_safe(zt, *c["rec"], w):        # (planted cases are all safe: tests/test_solve_ref.py)
                tally.setdefault("mask-unsafe", [0.0, 0])[1] += 1
            elif not np.array_equal(act[i], SR.expected_masks(zt, *c["rec"], w)):
                fails.append(f"{tag}: active[] differs from the masks of the truth")
    return fails
