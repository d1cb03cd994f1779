"""The margins of the rank rule of qpn_convexity_nodes (csrc/qpn_convexity.hip), measured on the CPU.

The kernel's pivoted Householder QR is replayed in float64 with the kernel's own summation order (every column norm and every
reflector dot product is one sequential sum, no fused multiply-add: csrc/build.sh compiles with -ffp-contract=off; only the
team's tree reduction inside `house` is replaced by a sequential sum).  On rows whose rank is known by construction it reports

  residue / thr        the largest remaining column norm once the true rank is exhausted, over min(k, n) eps sigma_max: above 1 the
                       threshold of Julia's rule alone takes one pivot too many
  residue / own        the same residue over sqrt(n) eps |a_c|, |a_c| the column's own original norm: the quantity CVX_DEP bounds
  pivot / own          the smallest genuine pivot |R_jj| over its column's original norm: what CVX_DEP sqrt(n) eps must stay below

over the nodes of tests/convexity_cases.py and over further draws: dependent pairs alone (k = 2), every row paired, and square
Gaussian rows (k = n, the worst conditioned rows test_gpu_convexity draws).  The GPU decides what the kernel does
(tests/test_gpu_convexity_reference.py asserts null_dim on every node); this tool is where the constant comes from.

    python tools/convexity_rank_margin.py [--draws 60]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import convexity_cases as CC  # noqa: E402
import convexity_ref as CR  # noqa: E402

EPS = np.finfo(float).eps


def replay(V, rank):
    """V [n, k] = Ae'.  -> (residue / thr, residue / (sqrt(n) eps own), smallest genuine pivot / own) with `rank` pivots taken."""
    V = V.copy()
    n, k = V.shape
    own = np.sqrt(np.sum(V * V, axis=0))
    vb = 1 + 0.5 * np.sin(0.7 * (np.arange(n) + 1))
    sig2 = 0.0
    for _ in range(30):
        p = V @ (V.T @ vb)
        nx, n0 = np.linalg.norm(p), np.linalg.norm(vb)
        if not (nx > 0 and n0 > 0):
            break
        sig2, vb = nx / n0, p / nx
    steps, thr, genuine = min(k, n), None, np.inf
    for j in range(steps):
        cn = np.zeros(k - j)
        for i in range(j, n):
            cn = cn + V[i, j:] * V[i, j:]
        best, pc = cn.max(), j + int(np.argmax(cn))
        if thr is None:
            thr = steps * EPS * max(np.sqrt(sig2), np.sqrt(best))
        if j == rank:
            return np.sqrt(best) / thr, float(np.max(np.sqrt(cn) / (np.sqrt(n) * EPS * own[j:]))), genuine
        genuine = min(genuine, np.sqrt(best) / own[pc])
        V[:, [j, pc]] = V[:, [pc, j]]
        own[[j, pc]] = own[[pc, j]]
        x = V[j:, j].copy()
        sig = 0.0
        for xi in x[1:]:
            sig += xi * xi
        if sig == 0.0:
            continue
        nrm = np.sqrt(x[0] * x[0] + sig)
        beta = -nrm if x[0] >= 0 else nrm
        tau = (beta - x[0]) / beta
        v = x * (1.0 / (x[0] - beta))
        v[0] = 1.0
        dot = np.zeros(k - j - 1)
        for i in range(n - j):
            dot = dot + v[i] * V[j + i, j + 1:]
        dot = dot * tau
        V[j:, j + 1:] -= np.outer(v, dot)
        V[j, j] = beta
    return 0.0, 0.0, genuine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=60)
    a = ap.parse_args()
    rows = {}

    def add(key, res):
        r = rows.setdefault(key, [0, 0.0, 0.0, np.inf, 0])
        r[0] += 1
        r[1], r[2], r[3] = max(r[1], res[0]), max(r[2], res[1]), min(r[3], res[2])
        r[4] += res[0] > 1

    for (n, m), nodes in CC.all_cases().items():
        for c in nodes:
            if c["scale"] == 0 and c["rank"] and c["family"] not in ("unit", "unit_pair", "zero_marked"):
                add((f"cases {c['family']}", n), replay(CR.selected_rows(c["A"], c["eq"]).T, min(c["rank"], n)))
    rng = np.random.default_rng(1)
    for n in (33, 64, 124, 129, 256):
        for _ in range(a.draws if n < 256 else a.draws // 3):
            x = rng.standard_normal(n)
            for f in (-1.0, 1.0, 2.0):
                add(("pair alone (k = 2)", n), replay(np.array([x, f * x]).T, 1))
    for n, r0 in ((64, 61), (128, 64), (256, 128), (256, 250)):
        for _ in range(4):
            P = rng.standard_normal((r0, n))
            add((f"every row paired (rank {r0})", n), replay(np.concatenate([P, -P]).T, r0))
    for n in (32, 128, 256):
        for _ in range(4):
            add(("Gaussian k = n (no dependence)", n), replay(rng.standard_normal((n, n)), n))
    print(f"{'rows':34s} {'n':>4s} {'nodes':>5s}  {'residue/thr':>11s} {'over thr':>8s}  {'residue/own':>11s}  {'pivot/own':>9s}")
    for (what, n), (cnt, rt, ro, g, over) in sorted(rows.items()):
        print(f"{what:34s} {n:4d} {cnt:5d}  {rt:11.2f} {over:8d}  {ro:11.3f}  {g:9.2e}")
    worst = max(r[2] for r in rows.values())
    least = min(r[3] for r in rows.values())
    print(f"worst residue / (sqrt(n) eps own) = {worst:.3f}; smallest genuine pivot / own = {least:.2e}; "
          f"CVX_DEP sqrt(256) eps = {8.0 * 16 * EPS:.2e}")


if __name__ == "__main__":
    main()
