"""Seeded box-MCPs (STD and GAVI rows) with a PLANTED, exactly known solution, and the cells of qpn_solve_avi_batch they run in.

plant() draws a state per row (tests/mcp_ref.py; each state at least once where N allows), the active residuals and
multipliers with magnitude in [0.5, 1.5], interior slacks and bound widths in [0.2, 1.5] (an infinite bound only on a side that
is not active), forms q := r* - M z* in longdouble and rounds it once; the active bounds are data.  The exact solution of the
ROUNDED data is then within cond * eps of the plant; truth() computes it (mcp_ref.solve_reference) and proves it by the
certificate.  The bound of a weak row (zero residual ON a bound) is then moved onto the truth, rounded to the feasible side: the
bound of a row whose z_i is an unknown does not enter the linear system, so the truth stays what it was and the row is exactly
feasible.

Families: sym (G G'/N + 0.2 I), skew (sym + 0.5 (S - S')/sqrt(N): M != M', a row/column-major mix-up shows), k1e4 (rotated
geometric spectrum 1 .. 1e-4, bitwise symmetric).
Kinds: box (kind = None), mixed (about 40 % GAVI rows, interleaved; row 0 is GAVI and row N - 1 a bounded STD row, so the shape
test of the Schur kernels -- leading free STD rows, then GAVI rows -- declines), swapped ([GAVI x m | free STD x n], the node
shape with its blocks exchanged: the ballot-mask test has to decline it), node ([free STD x n | GAVI x m]: scan_many only).
"""
from __future__ import annotations

import numpy as np

import mcp_ref as MR

LD = np.longdouble
INF = np.inf
FAMILIES = ("sym", "skew", "k1e4")
SUCCESS, RAY_TERM, MAX_ITERS, FAILURE = 1, 2, 3, 4

_P_STD = dict(lower=.22, upper=.22, interior=.25, free=.15, fixed=.08, weak=.08)
_P_GAVI = dict(at_l=.28, at_u=.28, inside=.25, open=.09, eq=.10)
_NODE_GAVI = dict(at_l=.3, at_u=.3, inside=.4)            # (the Schur kernels decline equality rows: not the shape's subject)


def _ld(a):
    return np.asarray(a, dtype=LD)


def matrix(rng, N, family):
    assert family in FAMILIES
    if family == "k1e4":
        V, _ = np.linalg.qr(rng.standard_normal((N, N)))
        M = (V * np.geomspace(1.0, 1e-4, N)) @ V.T
        return 0.5 * (M + M.T)                            # (a + b == b + a: bitwise symmetric)
    G = rng.standard_normal((N, N))
    M = G @ G.T / N + 0.2 * np.eye(N)
    if family == "skew":
        S = rng.standard_normal((N, N))
        M = M + 0.5 * (S - S.T) / np.sqrt(N)
    return M


def kind_vector(rng, N, kinds, nm=None):
    """None (box) or the uint8 kind vector of `kinds`; nm = (n, m) for swapped / node."""
    if kinds == "box":
        return None
    if kinds in ("swapped", "node"):
        n, m = nm
        assert n + m == N
        g, s = np.ones(m, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        return np.concatenate([g, s] if kinds == "swapped" else [s, g])
    assert kinds == "mixed"
    k = (rng.random(N) < 0.4).astype(np.uint8)
    k[0] = 1
    if N > 1:
        k[N - 1] = 0
    return k


def _draw_states(rng, rows, table):
    """A state per row of `rows`: each state of `table` once (in random rows) where there are enough rows, the rest drawn."""
    names, p = list(table), np.array(list(table.values()))
    out = list(rng.choice(names, size=len(rows), p=p / p.sum()))
    first = rng.permutation(len(rows))[:len(names)]
    for j, i in enumerate(first):
        out[i] = names[j]
    return out


def draw_states(rng, N, kind, kinds):
    state = np.empty(N, dtype="U8")
    g = np.zeros(N, dtype=bool) if kind is None else kind.astype(bool)
    if kinds in ("swapped", "node"):
        state[~g] = "free"
        state[g] = _draw_states(rng, np.flatnonzero(g), _NODE_GAVI)
        return state
    state[~g] = _draw_states(rng, np.flatnonzero(~g), _P_STD)
    state[g] = _draw_states(rng, np.flatnonzero(g), _P_GAVI)
    if kinds == "mixed" and N > 1 and state[N - 1] == "free":              # a BOUNDED STD row: another row's state, or a new one
        other = np.flatnonzero(~g & (state != "free"))
        if other.size:
            state[N - 1], state[other[0]] = state[other[0]], "free"
        else:
            state[N - 1] = rng.choice(["lower", "upper", "interior"])
    return state


def plant(rng, N, family, kinds, nm=None, M=None, kind=False, state=None):
    """One planted problem: dict(M, q, l, u, kind (None: box), state, plant (z*), family, kinds, N).  M, kind and the states
    may be given (the `shared` cell: one M and one kind vector, new states, q, l, u)."""
    M = matrix(rng, N, family) if M is None else M
    kind = kind_vector(rng, N, kinds, nm) if kind is False else kind
    state = draw_states(rng, N, kind, kinds) if state is None else state
    z, r = rng.standard_normal(N), rng.standard_normal(N)                  # inactive values where nothing below sets them
    l, u = np.full(N, -INF), np.full(N, INF)
    mag = lambda: rng.uniform(0.5, 1.5)
    gap = lambda: rng.uniform(0.2, 1.5)
    maybe = lambda v: v if rng.random() < 0.7 else None                    # (None: that side stays infinite)
    for i, s in enumerate(state):
        far_lo, far_hi = maybe(gap()), maybe(gap())
        if s in ("lower", "weak", "upper", "fixed"):                       # STD: z on a bound; weak rows sit on either side
            up = s == "upper" or (s == "weak" and rng.random() < 0.5)
            b = z[i]
            if s == "fixed":
                r[i] = rng.choice([-1, 1]) * mag()
                l[i], u[i] = b, b
            else:
                r[i] = 0.0 if s == "weak" else -mag() if up else mag()
                l[i], u[i] = ((b - far_lo if far_lo else -INF), b) if up else (b, (b + far_hi if far_hi else INF))
        elif s in ("at_l", "at_u", "eq"):                                  # GAVI: r on a bound, z the multiplier
            b = r[i]
            z[i] = mag() if s == "at_l" else -mag() if s == "at_u" else rng.choice([-1, 1]) * mag()
            l[i], u[i] = (b, b) if s == "eq" else (b, (b + far_hi if far_hi else INF)) if s == "at_l" else \
                ((b - far_lo if far_lo else -INF), b)
        elif s in ("interior", "inside"):                                  # strictly inside, at least one finite bound
            v = z[i] if s == "interior" else r[i]
            if far_lo is None and far_hi is None:
                far_lo = gap()
            l[i], u[i] = (v - far_lo if far_lo else -INF), (v + far_hi if far_hi else INF)
            if s == "interior":
                r[i] = 0.0
            else:
                z[i] = 0.0
        elif s == "free":
            r[i] = 0.0
        else:                                                              # open
            z[i] = 0.0
    q = np.asarray(_ld(r) - _ld(M) @ _ld(z), dtype=np.float64)
    c = dict(M=M, q=q, l=l, u=u, kind=kind, state=state, plant=z, family=family, kinds=kinds, N=N)
    _settle(c)
    return c


def data(c):
    """(M, q, l, u, kind) of a case: the leading arguments of mcp_ref's functions."""
    return c["M"], c["q"], c["l"], c["u"], c["kind"]


def _settle(c):
    """The truth of a new case (mcp_ref.solve_reference from the plant's states), kept with it; the bound of every weak row is
    moved onto the truth (see the module's docstring) and the point certified again, so the case's data are final from here."""
    zt, info = MR.solve_reference(*data(c), c["state"])
    weak = np.flatnonzero(c["state"] == "weak")
    if info["ok"] and weak.size:
        for i in weak:
            lower = abs(zt[i] - c["l"][i]) <= abs(zt[i] - c["u"][i])
            b = np.float64(zt[i])
            if lower and LD(b) > zt[i]:
                b = np.nextafter(b, -INF)
            if not lower and LD(b) < zt[i]:
                b = np.nextafter(b, INF)
            (c["l"] if lower else c["u"])[i] = b
        info["ok"], info["why"] = MR.certificate(zt, *data(c), c["state"])
    c["_truth"] = (zt, info)


def truth(c):
    """(z*, info): the exact solution of the case's rounded data and the certificate's verdict on it."""
    return c["_truth"]


def make_infeasible(c):
    """A copy of a case with GAVI rows made infeasible: two GAVI rows get the same row of M and the same q, and the disjoint
    ranges [0, 1] and [2, 3].  No z puts one value into both."""
    g = np.flatnonzero(c["kind"])
    assert g.size >= 2
    i, j = g[0], g[-1]
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items() if k != "_truth"}
    d["M"][j] = d["M"][i]
    d["q"][j] = d["q"][i]
    d["l"][[i, j]] = 0.0, 2.0
    d["u"][[i, j]] = 1.0, 3.0
    d["infeasible"] = True
    return d


# ---- the routes of qpn_solve_avi_batch (csrc/qpn_capi.hip, qpn_avi_reg.hip, qpn_avi_big.hip), restated ----------------------
REG_BS = ((8, 1), (16, 2), (32, 4), (40, 5), (48, 6), (56, 7), (64, 8))   # qpn_avi_reg_block_size: N <= limit -> BS
SCAN_BS = ((8, 1), (16, 2), (32, 4), (64, 8))                            # the avi_solve_reg_scan<BS> instantiations
BIG_ROWS, BIG_MAX = 256, 1024                                            # qpn_avi_big.hip: rows t, t + 256, ...; the ABI's limit
SCAN_GRID = 2048                                                         # blocks of a scan launch; 64 items per block and trip


def _leading_free(kind, l, u):
    free = (kind == 0) & (l == -INF) & (u == INF)
    return int(np.argmin(free)) if not free.all() else len(free)


def route_of(N, kind, l, u):
    """Which kernel solves an item, by the shape tests of the launchers: ("reg", BS) | ("schur",) | ("scan", BS) |
    ("big", rows per thread) | ("big_crash", rows per thread) | ("big_gated", rows per thread).  An item the Schur kernels keep
    by shape may still be handed on by their pivot test; nothing here depends on that."""
    assert 1 <= N <= BIG_MAX
    cls = -(-N // BIG_ROWS)
    if N <= 64:
        if kind is None or N < 2:
            return "reg", next(bs for lim, bs in REG_BS if N <= lim)
        n = _leading_free(kind, l, u)
        tail = kind[n:]
        node = n >= 1 and n <= 32 and N - n <= 32 and np.all(tail == 1) and not np.any(l[n:] == u[n:])
        # (free STD rows after a GAVI row make the free-row ballot something else than the low n bits)
        return ("schur",) if node else ("scan", next(bs for lim, bs in SCAN_BS if N <= lim))
    if kind is None:
        return "big", cls
    n = _leading_free(kind, l, u)
    node = 1 <= n <= 512 and 1 <= N - n <= 512 and np.all(kind[n:] == 1) and not np.any(l[n:] == u[n:])
    return ("big_crash" if node else "big_gated"), cls


# cell -> [(N, kinds, nm, items per family, families)]
_ALL = FAMILIES
CELLS = {
    "reg_box":    [(N, "box", None, 3, _ALL) for N in (1, 8, 9, 16, 17, 32, 33, 40, 41, 48, 49, 56, 57, 64)],
    "scan_mixed": [(N, "mixed", None, 3, _ALL) for N in (1, 2, 8, 9, 16, 17, 32, 33, 64)] +
                  [(9, "swapped", (5, 4), 3, _ALL), (64, "swapped", (32, 32), 3, _ALL)],
    "big_box":    [(N, "box", None, 3, _ALL) for N in (65, 256, 257)] + [(N, "box", None, 1, ("skew",)) for N in (513, 769, 1024)],
    "big_mixed":  [(N, "mixed", None, 3, _ALL) for N in (65, 130, 257)] + [(130, "swapped", (70, 60), 3, _ALL),
                                                                            (513, "mixed", None, 1, ("skew",))],
    "shared":     [(17, "box", None, 4, _ALL), (9, "mixed", None, 4, _ALL), (130, "box", None, 4, _ALL)],
}
# the route every item of a cell takes (N = 1 goes straight to the register kernel whatever its kind), by kinds
EXPECT = {"reg_box": "reg", "scan_mixed": "scan", "big_box": "big", "big_mixed": "big_gated"}

_CACHE = {}


def cell_cases(cell, seed=23):
    """[(N, kinds, family, [cases])] of one cell: one batch per shape and family (built once per process: the tests share them
    and leave them unchanged).  The `shared` cell's batches share one M and one kind vector."""
    if (cell, seed) not in _CACHE:
        out = []
        for N, kinds, nm, per, fams in CELLS[cell]:
            for f in fams:
                rng = np.random.default_rng([seed, sum(map(ord, cell + kinds + f)), N])
                if cell == "shared":
                    M, kind = matrix(rng, N, f), kind_vector(rng, N, kinds, nm)
                    cases = [plant(rng, N, f, kinds, nm, M=M, kind=kind) for _ in range(per)]
                else:
                    cases = [plant(rng, N, f, kinds, nm) for _ in range(per)]
                out.append((N, kinds, f, cases))
        _CACHE[cell, seed] = out
    return _CACHE[cell, seed]


def scan_many_nine(seed=23, count=4101):
    """4101 planted items of N = 9: every third one node-shaped (5 free STD + 4 GAVI rows: the Schur kernel keeps it), the
    others mixed (the scan kernel takes them: items g, g + 2048 and g + 4096 of one block).  Families in rotation."""
    if ("nine", seed, count) not in _CACHE:
        rng = np.random.default_rng([seed, 9])
        _CACHE["nine", seed, count] = [plant(rng, 9, FAMILIES[(i // 3 + i) % 3], "node" if i % 3 == 0 else "mixed", (5, 4))
                                       for i in range(count)]
    return _CACHE["nine", seed, count]


def scan_many_two(seed=23, distinct=16, count=64 * SCAN_GRID + 3):
    """(the 16 distinct planted mixed items of N = 2, the index of each of the 64 * 2048 + 3 items into them): tiled in
    rotation, so a block's 65th item -- the scan loop's second trip -- is compared with a known answer."""
    if ("two", seed) not in _CACHE:
        rng = np.random.default_rng([seed, 2])
        _CACHE["two", seed] = [plant(rng, 2, FAMILIES[i % 3], "mixed") for i in range(distinct)]
    return _CACHE["two", seed], np.arange(count) % distinct


def stack(cases, shared=False):
    """Cases of one size -> (M, q, l, u, kind) in math layout: M (batch, N, N) or, shared, (N, N); kind None, (batch, N) or,
    shared, (N,)."""
    M = cases[0]["M"] if shared else np.stack([c["M"] for c in cases])
    kind = None if cases[0]["kind"] is None else cases[0]["kind"] if shared else np.stack([c["kind"] for c in cases])
    return (M,) + tuple(np.stack([c[k] for c in cases]) for k in ("q", "l", "u")) + (kind,)


def oracle_solve(oracle, cases, shared=False, max_pivots=0, z0=None):
    """The CPU oracle (oracle/binding.py, handed in: this module does not import it) on a batch of cases."""
    M, q, l, u, kind = stack(cases, shared)
    o = oracle.default_opts()
    o.max_pivots = max_pivots
    return oracle.solve_avi_batch(M, q, l, u, z0=z0, kind=kind, opts=o)


def check_against_truth(cases, res, where, e_ref=None, factor=None):
    """One solver's outputs (dict of arrays: z, status, active) on `cases` against their truths -> (failure messages, worst
    error, items compared).  With e_ref (the oracle's worst error on the same cell and family) the accuracy bar is applied."""
    fails, worst, cnt = [], 0.0, 0
    z, st = np.asarray(res["z"]), np.asarray(res["status"])
    act = np.asarray(res["active"]) if res.get("active") is not None else None
    for i, c in enumerate(cases):
        zt, info = truth(c)
        tag = f"{where} [{i}] {c['family']} {c['kinds']} N={c['N']} cond={info['cond']:.1e}"
        if not info["ok"]:
            fails.append(f"{tag}: no certified truth ({info['why']})")
            continue
        if st[i] != SUCCESS:
            fails.append(f"{tag}: status {st[i]}")
            continue
        e = MR.mcp_error(z[i], zt)
        worst, cnt = max(worst, e), cnt + 1
        if e_ref is not None:
            bar = MR.SR.accuracy_bar(e_ref, factor or MR.SR.FACTOR)
            if not e <= bar:
                fails.append(f"{tag}: error {e:.3e} > bar {bar:.3e} (oracle {e_ref:.3e})")
        if act is not None and not np.array_equal(act[i], MR.expected_masks(zt, *data(c))):
            fails.append(f"{tag}: active[] differs from the masks of the truth")
    return fails, worst, cnt


# ---- planted non-solutions, the CSC entry, the checker's batches ------------------------------------------------------------
NONSOLUTION_SIZES = (9, 33, 64, 65, 257)


def nonsolution_batch(N, seed=23):
    """Four mixed items of one size; item 1 is planted infeasible (make_infeasible), items 0, 2 and 3 keep their truths."""
    if ("nonsol", N, seed) not in _CACHE:
        rng = np.random.default_rng([seed, 7, N])
        fam = FAMILIES[NONSOLUTION_SIZES.index(N) % 3]
        cases = [plant(rng, N, fam, "mixed") for _ in range(4)]
        cases[1] = make_infeasible(cases[1])
        _CACHE["nonsol", N, seed] = cases
    return _CACHE["nonsol", N, seed]


def crash_pivots(c):
    """The pivots of the crash (Stage A) on a case: one per free STD variable and one per equality GAVI row."""
    kind = np.zeros(c["N"], dtype=np.uint8) if c["kind"] is None else c["kind"]
    return int(np.sum((kind == 0) & (c["l"] == -INF) & (c["u"] == INF)) + np.sum((kind == 1) & (c["l"] == c["u"])))


def csc_case(N, seed=23):
    """A planted skew box item, thinned (|M_ij| < 0.3 -> 0, + 0.5 I), with one EMPTY column: the column of a fixed row (z_j = l_j
    = u_j is data, so M_jj = 0 costs no uniqueness -- mcp_ref.certificate asks positive definiteness of the other rows) -> (case,
    j, two 1-based CSC triples (colptr, rowval, nzval) of the same matrix: the first stores column j as explicit zeros and is
    otherwise canonical; the second leaves column j empty, stores one entry as two halves v/2 + v/2 (their sum is exact; the ABI
    adds duplicates) and stores one explicit zero elsewhere)."""
    if ("csc", N, seed) in _CACHE:
        return _CACHE["csc", N, seed]
    import scipy.sparse as sp
    rng = np.random.default_rng([seed, 5, N])
    M = matrix(rng, N, "skew")
    M[np.abs(M) < 0.3] = 0.0
    M += 0.5 * np.eye(N)
    state = draw_states(rng, N, None, "box")
    j = int(np.flatnonzero(state == "fixed")[0])
    M[:, j] = 0.0
    c = plant(rng, N, "skew", "box", M=M, kind=None, state=state)
    csc = sp.csc_matrix(M)
    csc.sort_indices()
    cols = [(list(csc.indices[csc.indptr[k]:csc.indptr[k + 1]]), list(csc.data[csc.indptr[k]:csc.indptr[k + 1]])) for k in range(N)]
    assert not cols[j][0]

    def pack(cols):
        ptr = np.cumsum([0] + [len(r) for r, _ in cols])
        return ((ptr + 1).astype(np.int32), np.array([i + 1 for r, _ in cols for i in r], dtype=np.int32),
                np.array([v for _, vs in cols for v in vs], dtype=np.float64))

    first = [(list(r), list(v)) for r, v in cols]
    first[j] = (list(range(N)), [0.0] * N)
    second = [(list(r), list(v)) for r, v in cols]
    k = next(k for k in range(N) if k != j and len(cols[k][0]) >= 2)               # split the column's last entry in two
    second[k][0].append(second[k][0][-1])
    half = second[k][1][-1] / 2
    second[k][1][-1] = half
    second[k][1].append(half)
    k2 = next(t for t in range(N) if t not in (j, k))                              # an explicit zero where M has none stored
    i0 = next(i for i in range(N) if i not in cols[k2][0])
    second[k2][0].insert(0, i0)
    second[k2][1].insert(0, 0.0)
    _CACHE["csc", N, seed] = (c, j, pack(first), pack(second))
    return _CACHE["csc", N, seed]


# size -> (family, shared M, shared kind): the three call forms of qpn_check_avi_batch between them
CHECK_FORMS = {24: ("sym", False, False), 64: ("skew", False, True), 65: ("k1e4", True, True), 257: ("skew", True, False)}


def check_batch(N, seed=23):
    """Three planted mixed items of one size in the call form CHECK_FORMS names -> (cases, shared M, shared kind)."""
    if ("check", N, seed) not in _CACHE:
        fam, sm, sk = CHECK_FORMS[N]
        rng = np.random.default_rng([seed, 3, N])
        M = matrix(rng, N, fam) if sm else None
        kind = kind_vector(rng, N, "mixed") if sk else False
        _CACHE["check", N, seed] = ([plant(rng, N, fam, "mixed", M=M, kind=kind) for _ in range(3)], sm, sk)
    return _CACHE["check", N, seed]


# (row state, what is moved, by how much, the flag of mcp_ref.check_degree it has to raise): the four violations of
# src/avi.jl:152-154 on an STD row (z_i moved: the other rows' residuals move with it) and on a GAVI row (q_i moved: r_i alone)
VIOLATIONS = (("lower", "z", +1e-3, 1), ("upper", "z", -1e-3, 2), ("lower", "z", -1e-3, 4), ("upper", "z", +1e-3, 8),
              ("at_l", "q", +1e-3, 1), ("at_u", "q", -1e-3, 2), ("at_l", "q", -1e-3, 4), ("at_u", "q", +1e-3, 8))


def violated(c, which):
    """(q, z, row): the case's q and its truth rounded to fp64, with one row moved as VIOLATIONS[which] says."""
    state, what, step, _ = VIOLATIONS[which]
    i = int(np.flatnonzero(c["state"] == state)[0])
    q, z = c["q"].copy(), np.asarray(truth(c)[0], dtype=np.float64)
    (q if what == "q" else z)[i] += step
    return q, z, i
