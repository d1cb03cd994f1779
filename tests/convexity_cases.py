"""Seeded nodes for qpn_convexity_nodes whose answer is known BY CONSTRUCTION: the rank of the selected rows always, the smallest
eigenvalue of Z' S Z in closed form where there is one (tests/convexity_ref.py encloses it everywhere).

A node is Qd = S/2 + K (K skew with small integer entries: exactly representable, and Qd + Qd' = S exactly for every family but
`rot`), the constraint rows A [m, n], the mask eq [m] of implicit equality rows, the true rank of the selected rows.

Hessian families (S):
  ident      c I, c in {2, -2, 0}
  diag       a permuted geometric diagonal 1 .. 1e-3 with one entry at -3
  blocks     block diagonal, blocks a I_s + b 11' of size s in {1, 2, 3}, zero coupling: eigenvalues a (s - 1 times) and a + s b,
             and a principal f x f part of a block has a (f - 1 times) and a + f b
  lap        the second-difference matrix tridiag(-1, 2, -1): tridiagonal already; with coordinates pinned it splits into runs of
             free coordinates, lambda_min = 2 - 2 cos(pi / (L + 1)) of the longest run L
  lap_dense  P lap P with the reflector P = I - (2/n) 11', n a power of two: dense, every entry exact, the spectrum of lap
  cluster    I - (1 - 2^-30) u u', u = 1/sqrt(n), n a power of 4: eigenvalue 1 (n - 1 times) and 2^-30; a principal f x f part has
             1 - (1 - 2^-30) f / n
  rot        U diag(lam) U', lam in [0.5, 2] and one eigenvalue at -tol (1 -+ 1e-2): the truth is the enclosure's alone

Row families (the selected rows; the other rows of A are Gaussian and unmarked):
  none, unit (distinct +-c e_i: Z' S Z is a principal submatrix), unit_pair (each unit row with its negative),
  dup_neg (a, -a), dup_same (a, a), dup_scaled (a, 2a) with dense Gaussian a -- variant 0 alone (k = 2), 1 next to r0 independent
  Gaussian rows, 2 every independent row paired --, int_comb (k <= 4 r0 small-integer combinations of r0 integer basis rows with
  entries in [-8, 8]: every sum exact), wide (the same with k >> n: k = 500 at n = 4 with rank 3, 4 and 2), zero_marked (all-zero
  rows with their mask bit set, next to unit rows).
Every cell (row family, shape) also holds two copies of its first nodes with S * 2^100, A * 2^-100 and S * 2^-100, A * 2^100:
powers of two are exact, so the truth scales exactly.

Condition on the inputs (asserted when a node is built; a draw that misses it is redrawn under the next seed): the first `rank`
singular values of the selected rows, and those of their independent part, satisfy sigma_min >= 1e-3 sigma_max.

Shapes: the smallest that cross each boundary of the kernel's size classes; slice_bytes / cvx_class / cvx_chunk restate
csrc/qpn_convexity.hip and every shape's class is asserted.
"""
from __future__ import annotations

import functools

import numpy as np

import convexity_ref as CR

LD = np.longdouble
PI = 4 * np.arctan(LD(1))                  # (np.pi is a float64)
TOL = 1e-6
SIGMA_RATIO = 1e-3
ALONE_DRAWS = 6                            # further draws of a dup_* pair alone per shape with n >= 64 (a third at n = 256)
N_MAX, M_MAX = 256, 1024

# ---- the size classes of csrc/qpn_convexity.hip, restated ---------------------------------------------------------------------
CVX_WAVES, CVX_GROUP = 4, 256
WAVE_SLICE_MAX, GROUP_SLICE_MAX, GLOBAL_CHUNK_BYTES = 40 << 10, 128 << 10, 512 << 20


def slice_bytes(n, m, T):
    """doubles S[n*n] V[n*m] tau vb p a b2 [n each] cn c0 [max(m,1) each] red[T], ints sel[max(m,1)] misc[4]; 16-byte rounded"""
    mm = max(m, 1)
    dbl = n * n + n * m + 5 * n + 2 * mm + T
    return (dbl * 8 + (mm + 4) * 4 + 15) & ~15


def cvx_class(n, m):
    if n <= 32 and slice_bytes(n, m, 64) <= WAVE_SLICE_MAX:
        return "wave"
    if n <= 128 and slice_bytes(n, m, CVX_GROUP) <= GROUP_SLICE_MAX:
        return "group"
    return "global"


def cvx_chunk(n, m):
    """nodes per launch of the global class"""
    return max(1, GLOBAL_CHUNK_BYTES // slice_bytes(n, m, CVX_GROUP))


M_WAVE_LAST = max(m for m in range(M_MAX + 1) if cvx_class(32, m) == "wave")
N_GROUP_LAST = max(n for n in range(1, 129) if cvx_class(n, 0) == "group")
SHAPES = (
    ((1, 0), "wave"), ((2, 2), "wave"), ((3, 4), "wave"), ((31, 16), "wave"), ((32, 32), "wave"), ((32, M_WAVE_LAST), "wave"),
    ((32, M_WAVE_LAST + 1), "group"), ((4, 1024), "group"), ((33, 66), "group"), ((64, 16), "group"), ((N_GROUP_LAST, 0), "group"),
    ((16, 1024), "global"), ((128, 0), "global"), ((129, 40), "global"), ((256, 256), "global"), ((256, 1024), "global"),
)
for (_n, _m), _c in SHAPES:
    assert cvx_class(_n, _m) == _c, (_n, _m, _c, cvx_class(_n, _m))
assert cvx_class(32, M_WAVE_LAST + 1) == "group" and cvx_class(N_GROUP_LAST + 1, 0) == "global" and 32 < M_WAVE_LAST < M_MAX

HESSIANS = ("ident", "diag", "blocks", "lap", "lap_dense", "cluster", "rot")
ROWS = ("none", "unit", "unit_pair", "dup_neg", "dup_same", "dup_scaled", "int_comb", "wide", "zero_marked")
DEPENDENT = ("unit_pair", "dup_neg", "dup_same", "dup_scaled", "int_comb", "wide")


def _pow(n, base):
    while n > 1 and n % base == 0:
        n //= base
    return n == 1


def hessian_fits(name, n):
    return {"lap_dense": n >= 2 and _pow(n, 2), "cluster": n >= 4 and _pow(n, 4)}.get(name, True)


def _lap(n):
    return 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


def _runs(free):
    """lengths of the runs of consecutive indices in the sorted list `free`"""
    out, run, prev = [], 0, None
    for i in free:
        if prev is not None and i == prev + 1:
            run += 1
        else:
            if run:
                out.append(run)
            run = 1
        prev = i
    return out + ([run] if run else [])


def hessian(name, n, rng, variant):
    """-> (S float64 exactly symmetric, lam_free: list of free coordinates -> lambda_min of S[free, free] as longdouble, or None
    where no closed form exists)."""
    if name == "ident":
        c = (2.0, -2.0, 0.0)[variant % 3]
        return c * np.eye(n), lambda free: LD(c)
    if name == "diag":
        d = np.concatenate([np.geomspace(1.0, 1e-3, n - 1), [-3.0]]) if n > 1 else np.array([-3.0])
        d = rng.permutation(d)
        return np.diag(d), lambda free: LD(d[list(free)].min())
    if name == "blocks":
        S, blocks, at = np.zeros((n, n)), [], 0
        while at < n:
            s = min(int(rng.integers(1, 4)), n - at)
            a, b = float(rng.integers(-2, 5)) / 2.0, float(rng.integers(-3, 4)) / 4.0
            S[at:at + s, at:at + s] = a * np.eye(s) + b
            blocks.append((at, s, a, b))
            at += s

        def lam_free(free):
            fs = set(free)
            best = np.inf
            for at, s, a, b in blocks:
                f = sum(i in fs for i in range(at, at + s))
                if f:
                    best = min(best, a + f * b, a if f >= 2 else np.inf)
            return LD(best)
        return S, lam_free
    if name == "lap":
        return _lap(n), lambda free: 2 - 2 * np.cos(PI / (max(_runs(sorted(free))) + 1))
    if name == "lap_dense":
        # n^2 P lap P = n^2 lap - 2n (1 w' + w 1') + 8 11' with w = lap 1 = e_1 + e_n, 1' lap 1 = 2: integers
        w = np.zeros(n); w[0] += 1.0; w[-1] += 1.0
        one = np.ones(n)
        S = (n * n * _lap(n) - 2 * n * (np.outer(one, w) + np.outer(w, one)) + 8 * np.outer(one, one)) / (n * n)
        return S, lambda free: (2 - 2 * np.cos(PI / (n + 1))) if len(free) == n else None
    if name == "cluster":
        g = 1.0 - 2.0 ** -30
        return np.eye(n) - (g / n) * np.ones((n, n)), lambda free: LD(1) - LD(g) * len(free) / n
    assert name == "rot"
    lam = rng.uniform(0.5, 2.0, n)
    lam[0] = -TOL * (1 - 1e-2 if variant % 2 == 0 else 1 + 1e-2)
    U, R = np.linalg.qr(rng.standard_normal((n, n)))
    S = (U * lam) @ U.T
    return 0.5 * (S + S.T), None


def _skew(rng, n):
    K = np.triu(rng.integers(-3, 4, (n, n)).astype(np.float64), 1)
    return K - K.T


def _int_rows(rng, k, r, n):
    """k rows that are small-integer combinations of r integer basis rows -> (rows, basis)"""
    B = rng.integers(-8, 9, (r, n)).astype(np.float64)
    C = rng.integers(-3, 4, (k, r)).astype(np.float64)
    C[~np.any(C != 0, axis=1), 0] = 1.0                   # (no all-zero combination: that is the zero_marked family)
    rows = C @ B
    assert np.all(np.any(rows != 0, axis=1))
    return rows, B


def rows(name, n, m, rng, variant):
    """-> dict(sel [k, n] the selected rows, rank, pinned: the coordinates the rows pin (None for dense rows), indep: the
    independent part, zeros: all-zero marked rows) or None where the family does not fit the shape."""
    d_target = (1, 2, max(1, n // 2))[variant]
    if name == "none":
        return dict(sel=np.zeros((0, n)), rank=0, pinned=[], indep=None, zeros=0)
    if name in ("unit", "unit_pair", "zero_marked"):
        zeros = min(3, m) if name == "zero_marked" else 0
        per = 2 if name == "unit_pair" else 1
        r = min(n - d_target, (m - zeros) // per)
        if r < 1 and not (zeros and r == 0):
            return None
        r = max(r, 0)
        coords = np.sort(rng.choice(n, r, replace=False))
        E = np.zeros((r, n))
        E[np.arange(r), coords] = rng.choice([1.0, -1.0, 0.5, -4.0], r)
        sel = np.concatenate([E, -E]) if per == 2 else E
        return dict(sel=sel, rank=r, pinned=list(coords), indep=E if r else None, zeros=zeros)
    if name.startswith("dup_"):
        f = {"dup_neg": -1.0, "dup_same": 1.0, "dup_scaled": 2.0}[name]
        if variant == 0:
            r0 = 1 if m >= 2 else 0
            part = rng.standard_normal((r0, n))
            sel = np.concatenate([part, f * part])
        elif variant == 1:
            r0 = min(n - 3 if n <= 64 else n // 2, m - 2)
            if r0 < 1:
                return None
            part = rng.standard_normal((r0 + 1, n))
            sel = np.concatenate([part, f * part[:1]])
            r0 += 1
        else:
            r0 = min(n // 2, m // 2)
            part = rng.standard_normal((r0, n))
            sel = np.concatenate([part, f * part])
        if r0 < 1:
            return None
        return dict(sel=sel, rank=r0, pinned=None, indep=part, zeros=0)
    if name == "int_comb":
        r0 = (1, min(n - 1, 3), min(max(n // 2, 1), 8))[variant]
        k = min(4 * r0, m)
        if r0 < 1 or k <= r0:
            return None
        sel, B = _int_rows(rng, k, r0, n)
        return dict(sel=sel, rank=r0, pinned=None, indep=B, zeros=0)
    assert name == "wide"
    if m < 8 * n or m < 64:
        return None
    k = min(m, 500 if n <= 4 else 1000)
    r0 = (n - 1, n, max(1, n // 2))[variant]
    if r0 < 1:
        return None
    sel, B = _int_rows(rng, k, r0, n)
    return dict(sel=sel, rank=r0, pinned=None, indep=B, zeros=0)


def sigma_ok(node):
    """the condition on the inputs: sigma_rank >= 1e-3 sigma_max on the selected rows and on their independent part"""
    for M, r in ((node["sel"], node["rank"]), (node["indep"], None if node["indep"] is None else node["indep"].shape[0])):
        if M is None or not r:
            continue
        sv = np.linalg.svd(M, compute_uv=False)
        if sv.size < r or not sv[r - 1] >= SIGMA_RATIO * sv[0]:
            return False
    return True


def make_node(hname, rname, n, m, variant, key):
    """One node; redrawn under the next seed until the condition on the inputs holds."""
    for attempt in range(50):
        rng = np.random.Generator(np.random.Philox(key=[attempt, key]))
        S, lam_free = hessian(hname, n, rng, variant)
        rw = rows(rname, n, m, rng, variant)
        if rw is None:
            return None
        k = rw["sel"].shape[0]
        assert k + rw["zeros"] <= m and rw["rank"] <= n
        A = rng.standard_normal((m, n))
        eq = np.zeros(m, np.uint8)
        pos = rng.permutation(m)[:k + rw["zeros"]]
        A[pos[:k]] = rw["sel"][rng.permutation(k)] if k else rw["sel"]
        A[pos[k:]] = 0.0
        eq[pos] = 1
        Qd = 0.5 * S + _skew(rng, n)
        node = dict(family=rname, hessian=hname, n=n, m=m, variant=variant, Qd=Qd, A=A, eq=eq, rank=rw["rank"],
                    sel=rw["sel"], indep=rw["indep"], scale=0, lam=None)
        if not sigma_ok(node):
            continue
        free = None if rw["pinned"] is None else [i for i in range(n) if i not in set(rw["pinned"])]
        if n - rw["rank"] == 0:
            node["lam"] = LD(np.inf)
        elif hname == "ident":
            node["lam"] = lam_free(None)                   # Z' (c I) Z = c I whatever the rows
        elif free is not None and lam_free is not None:
            node["lam"] = lam_free(free)
        return node
    raise AssertionError(f"no draw of {hname}/{rname} at ({n}, {m}) meets the condition on the inputs")


def scaled(node, e):
    """the node with S * 2^e and A * 2^-e (exact)"""
    out = dict(node, Qd=node["Qd"] * 2.0 ** e, A=node["A"] * 2.0 ** -e, sel=node["sel"] * 2.0 ** -e,
               indep=None if node["indep"] is None else node["indep"] * 2.0 ** -e, scale=e, base=node,
               lam=None if node["lam"] is None else node["lam"] * LD(2.0) ** e)
    out.pop("_truth", None)
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    """-> {(n, m): [node, ...]} in a fixed order.  Per shape and row family three variants (one at n = 256), the Hessian family
    rotating -- `none` and `unit` run through every Hessian family instead --, and two 2^+-100 copies per cell."""
    out = {}
    for si, ((n, m), cls) in enumerate(SHAPES):
        nodes = []
        for ri, rname in enumerate(ROWS):
            cell = []
            if rname in ("none", "unit"):
                plan = [(h, hi % 3) for hi, h in enumerate(HESSIANS)]
            else:
                plan = [(HESSIANS[(si + ri + v) % len(HESSIANS)], v) for v in range(3)]
            if n == N_MAX:
                plan = plan[(si + ri) % len(plan):][:1] if rname not in ("none", "unit") else plan[:2]
            if rname.startswith("dup_") and n >= 64:
                # k = 2 at a large n is where min(k, n) eps sigma_max underestimates a Householder sweep's residue, and one
                # draw in five crosses it: the pair alone is drawn several times
                plan = plan + [(HESSIANS[(si + ri + v) % 4], 0) for v in range(ALONE_DRAWS if n < N_MAX else ALONE_DRAWS // 3)]
            for pi, (h, v) in enumerate(plan):
                while not hessian_fits(h, n):
                    h = HESSIANS[(HESSIANS.index(h) + 1) % len(HESSIANS)]
                node = make_node(h, rname, n, m, v, key=1000 * si + 10 * ri + pi)
                if node is not None:
                    cell.append(node)
            if cell and n < N_MAX:
                cell += [scaled(cell[0], 100), scaled(cell[-1], -100)]
            nodes += cell
        if cls == "wave" and len(nodes) % CVX_WAVES == 0:          # a wave-class batch ends in a partly filled workgroup
            nodes.append(make_node("lap", "none", n, m, 0, key=1000 * si + 999))
        assert nodes and (cls != "wave" or len(nodes) % CVX_WAVES)
        out[(n, m)] = nodes
    return out


def snorm(node):
    S = node["Qd"] + node["Qd"].T
    return float(np.linalg.norm(S, 2))


def truth(node):
    """dict(lo, hi, d, snorm, e64): the enclosure of convexity_ref.reference, |S|_2, and plain64's distance from the enclosure
    over |S|_2.  Computed once per node and kept with it; a 2^e copy takes its base's enclosure times 2^e (exact)."""
    if "_truth" in node:
        return node["_truth"]
    sn = snorm(node)
    if node["scale"]:
        b = truth(node["base"])
        f = LD(2.0) ** node["scale"]
        lo, hi, d = b["lo"] * f, b["hi"] * f, b["d"]
    else:
        lo, hi, d = CR.reference(node["Qd"], node["sel"], node["rank"])
    p, pd = CR.plain64(node["Qd"], node["sel"], node["rank"])
    assert pd == d
    e64 = 0.0 if d == 0 else CR.dist(p, lo, hi) / max(sn, CR.UNDERFLOW)
    node["_truth"] = dict(lo=lo, hi=hi, d=d, snorm=sn, e64=e64)
    return node["_truth"]


def stack(nodes):
    """-> (Qc [b, n, n], Ac [b, n, m], eq [b, m]) in the engine's layout (column-major blocks)"""
    n, m = nodes[0]["n"], nodes[0]["m"]
    Qc = np.ascontiguousarray(np.swapaxes(np.stack([c["Qd"] for c in nodes]), 1, 2))
    Ac = np.ascontiguousarray(np.swapaxes(np.stack([c["A"] for c in nodes]), 1, 2)) if m else np.zeros((len(nodes), n, 0))
    eq = np.stack([c["eq"] for c in nodes]) if m else np.zeros((len(nodes), 0), np.uint8)
    return Qc, Ac, eq
