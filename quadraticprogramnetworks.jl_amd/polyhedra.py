"""Batched polyhedral primitives on the node-AVI path (first step).

The reference answers `isempty(poly)` / `exemplar(poly)` (src/sets.jl:591-655) with one OSQP LP per polyhedron --
thousands of tiny independent solves inside `remove_subsets` (:889-902) and the intersection tree
(src/intersection.jl:66-105).  Here a whole batch of closed polyhedra {x : l <= A x <= u} goes through ONE call of
the node solver: the projection of the origin,

        min 1/2 |x|^2   s.t.  l <= A x <= u,

is a strictly convex QP whose KKT system is exactly a node's reduced AVI with Q = I, q = 0 (src/avi.jl:205-251), so
    status SUCCESS   <=>  the polyhedron is non-empty, and x is its minimum-norm point (an exemplar),
    status RAY_TERM  <=>  it is empty (the feasibility LP has no solution: a secondary ray).
Polyhedra of different sizes share a batch: missing rows are padded with 0'x in (-inf, inf), missing variables with
unconstrained ones (their minimum-norm value is 0).

exemplar_batch / isempty_batch (minimum-norm member, closed bounds) are the fast primitives behind issubset_batch and
remove_subsets.  The reference's own decision rule -- the slack-minimising LP of `exemplar` (src/sets.jl:591-642) with its
tolerance bands and open bounds (rl / ru, :68-92, :354-356) -- is exemplar_slack_batch / isempty_slack_batch, and
implicit_bounds_batch is `implicit_bounds` (:660-713): all of them LPs over the same rows, i.e. node-AVIs with Q = 0, batched
through the same node solver (the general kernels take them: an LP's H block has no pivots for the matrix-core path).

On an engine with `solve_lps` (qpn_solve_lps, a batched simplex with the outcomes OPTIMAL / INFEASIBLE / UNBOUNDED and a certificate
for each) the LPs of exemplar_slack_batch and implicit_bounds_batch are jobs over shared polyhedra, and on one with
`issubset_pairs` (qpn_issubset_pairs) a subset question P1 ⊆ P2 is ONE job: the crash and phase 1 over P1 once, then the finite
bounds of P2 as objectives one after the other, from the basis the previous one left, until one refutes; issubset_batch packs the
distinct polyhedra by shape and builds no query.  solve_lps_host and issubset_pairs_host are the numpy twins of the two entries:
the normative statements of their methods, to which the kernels are bit-equal.  An engine without the methods (the oracle engine)
keeps the node-AVI route.  On an engine with `exemplar_polys` (qpn_exemplar_polys) the emptiness question of a polyhedron whose
bounds may be open is ONE job too, opt-in through route="polyhedron": the job expands the slack LP, solves it and applies the
reference's rule to its own duals (exemplar_polys_host is the twin).  On one with `exemplar_products` (qpn_exemplar_products) the
products of pieces of the intersection tree are jobs over one pool of rows (isempty_products; exemplar_products_host is the twin).
On one with `intersection_trees` (qpn_intersection_trees) the tree itself is walked on the device, the empty prefixes pruned depth by
depth (intersection_trees; intersection_trees_host is the twin).
On one with `irredundant_bounds` (qpn_irredundant_bounds) irredundant_batch removes the bounds of polyhedra that their other bounds
imply, one job per polyhedron (irredundant_bounds_host is the twin); there is no other route for it.

These are the batch front ends: they normalise their inputs (_triple), pick a route, pack by shape (pack_by_shape), call the
engine and unpack.  The numpy twins and the result codes are polyhedra_host.py; their public names stay importable from here.
"""
from __future__ import annotations

import itertools

import numpy as np

from .polyhedra_host import *  # noqa: F401,F403  (the twins, the codes, INF: every public name of theirs is a name of this module)


# ---- what every front end does: normalise, pack by shape, call the node solver ----------------------------------------------
def _triple(p, cache=None):
    """An object with `vectorize() -> (A, l, u)` (programs.Poly) or an (A, l, u) triple -> (A float64 [rows, columns], l, u
    float64 [rows]).  cache: a dict of the call, by id (the same object shows up in many pairs); it keeps the object alive.
    A level asks tens of thousands of these: an array that has its shape already is not reshaped."""
    if cache is not None and id(p) in cache:
        return cache[id(p)][0]
    A, l, u = p.vectorize() if hasattr(p, "vectorize") else p
    A = np.asarray(A, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    if A.ndim != 2:
        A = np.atleast_2d(A)
    got = (A, l if l.ndim == 1 else l.reshape(A.shape[0]), u if u.ndim == 1 else u.reshape(A.shape[0]))
    if cache is not None:
        cache[id(p)] = (got, p)
    return got


def _by_shape(keyed, beyond=None):
    """Positions grouped by shape.  keyed: (position, shape) in input order; beyond(shape): the shapes a kernel does not take.
    -> ([(shape, positions)]: the shapes in sorted order, the positions of each in input order; the positions beyond)."""
    groups = {}
    for b, shape in keyed:
        groups.setdefault(shape, []).append(b)
    out_of = [shape for shape in groups if beyond is not None and beyond(shape)]       # (asked once per shape, not per item)
    return sorted((shape, bs) for shape, bs in groups.items() if shape not in out_of), sorted(b for shape in out_of for b in groups[shape])


def _stack(trips, extras=()):
    """Triples of one shape -> (A [k, r, d], l [k, r], u [k, r]) and the per-item `extras` ([k] sequences of [r]) stacked alike."""
    return tuple(np.stack([t[c] for t in trips]) for c in range(3)) + tuple(np.stack(e) for e in extras)


def pack_by_shape(trips, items=None, extras=(), beyond=None):
    """The packs of the batched entries: `items` (positions in `trips`, normalised triples; default: all) packed by shape
    (rows, columns), shapes sorted, members in input order.  extras: per-position sequences of [rows] arrays (the open flags)
    stacked with them; beyond((rows, columns)): the shapes that go another way.
    -> ([((r, d), members, A [k, r, d], l [k, r], u [k, r], *extras [k, r])], the items beyond)."""
    items = range(len(trips)) if items is None else items
    groups, out_of = _by_shape(((b, trips[b][0].shape) for b in items), beyond)
    return [(shape, members) + _stack([trips[b] for b in members], [[e[b] for b in members] for e in extras])
            for shape, members in groups], out_of


def _has(engine, method):
    return callable(getattr(engine, method, None))


class without:
    """without(engine, *names): the engine with the methods `names` hidden, for the route of an engine that lacks them."""

    def __init__(self, eng, *names):
        self._eng, self._names = eng, names

    def __getattr__(self, name):
        if name in self._names:
            raise AttributeError(name)
        return getattr(self._eng, name)


def _padded(trips, m, d):
    """Polyhedra of different sizes in one batch of the node solver: -> (A [B, m, d], l, u [B, m]) with missing rows 0'x in
    (-inf, inf) and missing variables in no row."""
    B = len(trips)
    A = np.zeros((B, m, d)); l = np.full((B, m), -INF); u = np.full((B, m), INF)
    for b, (Ab, lb, ub) in enumerate(trips):
        r, c = Ab.shape
        A[b, :r, :c] = Ab; l[b, :r] = lb; u[b, :r] = ub
    return A, l, u


def node_qp(Q, cost, A, l, u, engine):
    """Batch of  min 1/2 x'Q_b x + cost_b'x  s.t.  l_b <= A_b x <= u_b  (padded arrays A [B, m, d]; Q None: LPs, Q = 0) as nodes
    through `solve_nodes` (the HIP engine: fused assembly + solve) or, on an engine without it, `solve_avi_batch`.
    -> (status [B] int32, z [B, d + m]: x, then the rows' multipliers)."""
    B, m, d = A.shape
    if hasattr(engine, "solve_nodes"):
        from .engine import colmajor
        res = engine.solve_nodes(colmajor(np.zeros((B, d, d)) if Q is None else Q), np.zeros((B, d, 1)), cost, colmajor(A),
                                 np.zeros((B, m, 1)), l, u, np.zeros(1))
    else:
        M = np.zeros((B, d + m, d + m))
        if Q is not None:
            M[:, :d, :d] = Q
        M[:, :d, d:] = -np.swapaxes(A, 1, 2); M[:, d:, :d] = A
        lo = np.concatenate([np.full((B, d), -INF), l], axis=1); hi = np.concatenate([np.full((B, d), INF), u], axis=1)
        kind = np.concatenate([np.zeros((B, d), np.uint8), np.ones((B, m), np.uint8)], axis=1)
        res = engine.solve_avi_batch(np.swapaxes(M, 1, 2), np.concatenate([cost, np.zeros((B, m))], axis=1), lo, hi, kind=kind)
    return np.asarray(res["status"]).astype(np.int32), np.asarray(res["z"])


def exemplar_batch(polys, engine):
    """-> (empty [B] bool, example [B] list of x or None, status [B] int32).

    `polys`: sequence of objects with `vectorize() -> (A, l, u)` (programs.Poly) or (A, l, u) triples.
    `engine`: anything with `solve_nodes` (the HIP engine: fused assembly + solve) or `solve_avi_batch`."""
    trips = [_triple(p) for p in polys]
    B = len(trips)
    if B == 0:
        return np.zeros(0, bool), [], np.zeros(0, np.int32)
    d = max(1, max(t[0].shape[1] for t in trips))
    A, l, u = _padded(trips, max(1, max(t[0].shape[0] for t in trips)), d)
    status, z = node_qp(np.broadcast_to(np.eye(d), (B, d, d)).copy(), np.zeros((B, d)), A, l, u, engine)
    empty = status != 1
    example = [None if empty[b] else z[b, : trips[b][0].shape[1]].copy() for b in range(B)]
    return empty, example, status


def isempty_batch(polys, engine):
    """`isempty(poly)` (src/sets.jl:649-655) for a whole batch: True where {x : l <= A x <= u} has no point.
    Raises if the solver ended in anything but SUCCESS / RAY_TERM for an item (its answer would be a guess)."""
    empty, _, status = exemplar_batch(polys, engine)
    bad = np.nonzero((status != 1) & (status != 2))[0]
    if bad.size:
        raise RuntimeError(f"isempty_batch: solver status {status[bad[0]]} on item {int(bad[0])}")
    return empty


def issubset_batch(pairs, engine, tol=1e-6):
    """`P1 ⊆ P2` (src/sets.jl:376-407) for a batch of pairs -> bool [len(pairs)].

    The reference minimises +-a'x over P1 for every finite bound of P2 (one OSQP LP each) and answers false when a
    minimum falls below the bound by more than `tol` or the LP is unbounded.  Equivalently: P1 ⊆ P2 iff, for every
    finite bound of P2, P1 intersected with the closed half-space beyond that bound (moved out by `tol`) is EMPTY --
    one emptiness query per bound, all pairs and bounds in one `isempty_batch` call.  An empty P1 is a subset of
    anything (the reference's LP is infeasible there and it answers false; noted, not mirrored).

    An engine with `issubset_pairs` (qpn_issubset_pairs) takes a pair as ONE job instead: the distinct polyhedra are packed by
    shape, a call per pair of shapes, and no query is built (_issubset_pairs_route).  It compares the minimum with the bound
    where the queries ask for emptiness beyond it: the verdicts can differ only where the minimum lies within rounding of
    l2 - tol, and either verdict is sound there."""
    if len(pairs) and _has(engine, "issubset_pairs"):
        return _issubset_pairs_route(pairs, engine, tol)
    queries, owner = [], []
    keyed = {}                                   # per polyhedron (the same object shows up in many pairs): its rows as hashable keys

    def rows_of(P):
        got = keyed.get(id(P))
        if got is None:
            A, l, u = _triple(P)
            Ar = np.round(A, 9) + 0.0
            got = keyed[id(P)] = (A, l, u, [Ar[r].tobytes() for r in range(A.shape[0])])
        return got

    for k, (P1, P2) in enumerate(pairs):
        A1, l1, u1, k1 = rows_of(P1)
        A2, l2, u2, k2 = rows_of(P2)
        # a bound of P2 that P1 carries itself -- the same normal (to 1e-9) with a bound at least as tight -- holds on all of P1: no LP
        own = {}
        for r, key in enumerate(k1):
            own.setdefault(key, []).append(r)
        for i in range(A2.shape[0]):
            mine = own.get(k2[i], ())
            lo1 = max((l1[r] for r in mine), default=-INF); hi1 = min((u1[r] for r in mine), default=INF)
            if np.isfinite(l2[i]) and not lo1 >= l2[i] - tol:          # a violation is a point of P1 with a'x <= l2 - tol
                queries.append((np.vstack([A1, A2[i:i + 1]]), np.append(l1, -INF), np.append(u1, l2[i] - tol))); owner.append(k)
            if np.isfinite(u2[i]) and not hi1 <= u2[i] + tol:          # ... or with a'x >= u2 + tol
                queries.append((np.vstack([A1, A2[i:i + 1]]), np.append(l1, u2[i] + tol), np.append(u1, INF))); owner.append(k)
    out = np.ones(len(pairs), bool)
    if queries:
        # a query the solver neither answers with a point (SUCCESS) nor with a ray (RAY_TERM: empty) counts against the subset
        # claim, as the reference's `ret.info.status_val != 1 -> return false` does (src/sets.jl:397-398): the piece is kept
        _, _, status = exemplar_batch(queries, engine)
        for st, k in zip(status, owner):
            if st != 2:
                out[k] = False
    return out


def remove_subsets(polys, engine, tol=1e-6):
    """`remove_subsets(pu::PolyUnion)` (src/sets.jl:889-902): drop every polyhedron that is a subset of another one
    still kept, scanning in order like the reference; all k (k - 1) subset tests run as one batch first.
    -> (kept polys, is_subset mask)."""
    k = len(polys)
    idx = [(i, j) for i in range(k) for j in range(k) if i != j]
    sub = np.zeros((k, k), bool)
    if idx:
        res = issubset_batch([(polys[i], polys[j]) for i, j in idx], engine, tol=tol)
        for (i, j), r in zip(idx, res):
            sub[i, j] = r
    is_subset = np.zeros(k, bool)
    for i in range(k):
        if any(j != i and not is_subset[j] and sub[i, j] for j in range(k)):
            is_subset[i] = True
    return [p for p, s in zip(polys, is_subset) if not s], is_subset


def subset_packs(pairs):
    """The calls of issubset_pairs that answer `pairs`: the distinct polyhedra (by id: the same object shows up in many pairs) are
    packed by shape (rows, columns), first and second pieces apart, and every pair of shapes is one call with its index arrays
    into the two packs.  -> ([(positions in pairs, (A1c, l1, u1, A2c, l2, u2, pi, pj))], positions beyond the kernel's limits)."""
    from .engine import colmajor
    trips = {}

    def shapes():
        for k, (P1, P2) in enumerate(pairs):
            s1, s2 = _triple(P1, trips)[0].shape, _triple(P2, trips)[0].shape
            if s1[1] != s2[1]:
                raise ValueError(f"issubset_batch: pair {k} has polyhedra in {s1[1]} and {s2[1]} variables")
            yield k, (s1, s2)

    groups, beyond = _by_shape(shapes(), lambda s: max(s[0][0], s[1][0]) > LP_MAX_R or s[0][1] > LP_MAX_D or min(s[0] + s[1]) < 1)
    calls = []
    for _, ks in groups:
        packs = ({}, {})                                     # id -> position, first and second pieces
        idx = np.empty((2, len(ks)), np.int32)
        for t, k in enumerate(ks):
            for side in (0, 1):
                idx[side, t] = packs[side].setdefault(id(pairs[k][side]), len(packs[side]))
        arrs = ()
        for side in (0, 1):
            A, l, u = _stack([trips[i][0] for i in packs[side]])  # (insertion order = position)
            arrs += (colmajor(A), l, u)
        calls.append((ks, arrs + (idx[0].copy(), idx[1].copy())))
    return calls, beyond


def _issubset_pairs_route(pairs, engine, tol):
    """issubset_batch on an engine with `issubset_pairs`: one call per pair of shapes (subset_packs), `sub` is the answer.  A
    shape beyond the kernel's limits keeps the route of the emptiness queries."""
    calls, beyond = subset_packs(pairs)
    out = np.ones(len(pairs), bool)
    for ks, args in calls:
        out[ks] = _to_host(engine.issubset_pairs(*args, tol=tol)["sub"]).astype(bool)
    if beyond:
        out[beyond] = issubset_batch([pairs[k] for k in beyond], without(engine, "issubset_pairs"), tol=tol)
    return out


LP_CHUNK_BYTES = 1 << 30          # padded input of one batched LP call (host arrays; the device copy is as large again)


def issubset_batch_chunked(pairs, engine, tol=1e-6, chunk_bytes=None):
    """issubset_batch with the batch cut into calls whose padded host arrays stay below chunk_bytes (a level of a large net
    asks millions of subset questions; one call for all of them would need their padded copies all at once).  On an engine with
    `issubset_pairs` a call's arrays are the packs of its distinct polyhedra and two indices per pair: those bytes are counted."""
    chunk_bytes = chunk_bytes or LP_CHUNK_BYTES
    out = np.ones(len(pairs), bool)
    packed = _has(engine, "issubset_pairs")                       # that route uploads every distinct polyhedron of a call once
    start, trips = 0, {}
    while start < len(pairs):
        cost, stop, seen = 0, start, set()
        while stop < len(pairs):
            (A1, _, _), (A2, l2, u2) = [_triple(P, trips) for P in pairs[stop]]
            rows1, d = A1.shape
            if packed:
                c = 8                                        # its two indices; a polyhedron counts where it first shows up
                for side, (P, A) in enumerate(zip(pairs[stop], (A1, A2))):
                    if (side, id(P)) not in seen:
                        c += (A.size + 2 * A.shape[0]) * 8
            else:
                nq = int(np.isfinite(l2).sum() + np.isfinite(u2).sum())
                c = nq * ((rows1 + 1) * d + d * d + 4 * (rows1 + 1 + d)) * 8
            if stop > start and cost + c > chunk_bytes:
                break
            cost += c; stop += 1
            if packed:
                seen.update((side, id(P)) for side, P in enumerate(pairs[stop - 1]))
        out[start:stop] = issubset_batch(pairs[start:stop], engine, tol=tol)
        start = stop
    return out


PAIR_CHUNK = 1 << 22             # (member, piece) pairs of one members_outside call of remove_subsets_many, about
REFUTE_ROUTE = "pairs"           # how remove_subsets_many puts members to pieces on an engine: "pairs" = members_outside over pair
                                 # lists made here; "lists" = members_outside_lists, the pairs enumerated on the device (opt-in)


def _on_device(engine):
    return getattr(engine, "device", -1) >= 0


def _interior_member_groups(trips, engine, delta=1e-2, chunk=20000):
    """interior_members_batch's work: the queries packed by size (rows, columns), one engine call per pack of at most `chunk`.
    -> list of dict(idx: positions in `trips`, x [B, d], ok [B], and with an engine that has interior_members also Ac [B, d, r],
    l, u [B, r]: the pack as the engine got it).  x and ok stay where the engine left them (device tensors on a device engine)."""
    fused = _has(engine, "interior_members")
    out = []
    for (_, d), idx_all, A_all, l_all, u_all in pack_by_shape([_triple(t) for t in trips])[0]:
        for c0 in range(0, len(idx_all), chunk):
            idx = idx_all[c0:c0 + chunk]
            B = len(idx)
            A, l, u = A_all[c0:c0 + chunk], l_all[c0:c0 + chunk], u_all[c0:c0 + chunk]
            if fused:
                # the engine makes the records itself (qpn_interior_members): only the polyhedra go to it
                from .engine import colmajor
                ne, nlo, nhi = interior_member_counts(l, u)
                if _on_device(engine):
                    import torch
                    dv = f"cuda:{engine.device}"
                    A, l, u = (torch.as_tensor(a, dtype=torch.float64, device=dv) for a in (A, l, u))
                Ac = colmajor(A)
                x, ok, _ = engine.interior_members(Ac, l, u, delta, ne, nlo, nhi)
                out.append(dict(idx=idx, x=x, ok=ok, Ac=Ac, l=l, u=u))
                continue
            Qc, qd, Ac, ll, uu = interior_member_records(A, l, u, delta)
            nf, mp = qd.shape[1], ll.shape[1]
            res = engine.solve_nodes(Qc, np.zeros((B, 1, nf)), qd, Ac, np.zeros((B, 1, mp)), ll, uu, np.zeros(1))
            st = np.asarray(res["status"]); z = np.asarray(res["z"])
            out.append(dict(idx=idx, x=z[:, :d], ok=(st == 1) & (z[:, d] <= 1e-6)))
    return out


def _to_host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def interior_members_batch(trips, engine, delta=1e-2, chunk=20000):
    """One member per polyhedron (A, l, u), well inside its INEQUALITY rows: the slack program of `exemplar` (src/sets.jl:608-619)
    with the equality rows (l == u) kept as equalities -- a lower-dimensional piece gets a point of its relative interior instead
    of eps = 0 at an arbitrary feasible point -- and a small proximal term,

        min  eps + delta/2 (|x|^2 + eps^2)   s.t.  a_i'x = l_i (equality rows),  a_i'x + eps >= l_i,  a_i'x - eps <= u_i (the others),

    so that every query is a strictly convex node: with the equality multipliers in the free block (level_batch.free_equalities)
    the fused node kernels take it, where the plain LP -- no pivots in its H block -- fell to the general kernel, the slowest
    call of a level's sweep.  The proximal term caps the slack at 1 / delta and picks the least-norm point among the deepest ones;
    the answer is used as ONE member of the polyhedron (remove_subsets_many), never as an optimum.
    Queries over polyhedra of one size (rows, columns) are packed together: a level asks tens of thousands of them, a Python loop
    per record costs more than their solve.  An engine with `interior_members` gets the polyhedra and makes the records on the
    device (qpn_interior_members); any other gets the records from interior_member_records through solve_nodes.
    -> list of x or None (empty / no answer)."""
    out = [None] * len(trips)
    for g in _interior_member_groups(trips, engine, delta, chunk):
        x = _to_host(g["x"]); ok = _to_host(g["ok"]).astype(bool)
        for k in np.nonzero(ok)[0]:
            out[g["idx"][k]] = x[k].copy()
    return out


def _refuted_by_members(comp, flat, starts, engine, tol):
    """remove_subsets_many's refutation matrices on an engine with `members_outside`: the members stay where the solve left
    them, every (rows, columns) pack of second pieces is ONE members_outside call over the pack as interior_members got it, and
    only the verdicts come to the host.  -> {list a: refuted [k, k] bool}."""
    if REFUTE_ROUTE not in ("pairs", "lists"):
        raise ValueError(f"polyhedra.REFUTE_ROUTE: unknown route {REFUTE_ROUTE!r}")
    by_lists = REFUTE_ROUTE == "lists" and _has(engine, "members_outside_lists")
    groups = _interior_member_groups(flat, engine)
    nflat = len(flat)
    grp_of = np.zeros(nflat, np.int64); pos_of = np.zeros(nflat, np.int64); xrow = np.zeros(nflat, np.int64)
    ok_h = np.zeros(nflat, bool)
    X_of, rows_d = {}, {}                                   # per member dimension d: the packs' members, one after the other
    for g, grp in enumerate(groups):
        idx = np.asarray(grp["idx"], dtype=np.int64)
        d = int(grp["x"].shape[1])
        grp_of[idx] = g; pos_of[idx] = np.arange(len(idx)); xrow[idx] = rows_d.get(d, 0) + np.arange(len(idx))
        rows_d[d] = rows_d.get(d, 0) + len(idx)
        if not by_lists:                                    # (the lists route leaves the flags where they are)
            ok_h[idx] = _to_host(grp["ok"]).astype(bool)
        X_of.setdefault(d, []).append(grp["x"])
    dev = _on_device(engine)
    if dev:
        import torch
    cat = (lambda xs: xs[0] if len(xs) == 1 else torch.cat(xs)) if dev else (lambda xs: xs[0] if len(xs) == 1 else np.concatenate(xs))
    X_of = {d: cat(xs) for d, xs in X_of.items()}
    if by_lists:
        return _refuted_by_lists(comp, starts, engine, tol, groups, xrow, X_of, cat)
    refuted = {a: np.zeros((len(trips), len(trips)), bool) for a, trips in enumerate(comp) if trips is not None}

    def ask(blocks):
        """One members_outside call per pack for the pairs of `blocks` [(list a, ii, jj)]; the verdicts go into refuted[a]."""
        FI = np.concatenate([starts[a] + ii for a, ii, _ in blocks]); FJ = np.concatenate([starts[a] + jj for a, _, jj in blocks])
        verdict = np.zeros(len(FI), bool)
        gj = grp_of[FJ]
        for g in np.unique(gj).tolist():
            grp = groups[g]
            sel = np.nonzero(gj == g)[0]
            pi = xrow[FI[sel]].astype(np.int32); pj = pos_of[FJ[sel]].astype(np.int32)
            if dev:
                pi, pj = (torch.as_tensor(v, device=grp["x"].device) for v in (pi, pj))
            Ac = grp["Ac"]
            out = engine.members_outside(Ac, grp["l"], grp["u"], X_of[int(Ac.shape[1])], pi, pj, 10 * tol)
            verdict[sel] = _to_host(out).astype(bool)
        verdict &= ok_h[FI]                                 # (no member for the first piece: nothing is refuted by it)
        p0 = 0
        for a, ii, jj in blocks:
            refuted[a][ii, jj] = verdict[p0:p0 + len(ii)]
            p0 += len(ii)

    # every ordered pair (first piece i, second piece j), i != j, of every list, ordered by the second piece -- the kernel reads a
    # piece once for a run of pairs that share it -- and asked in slices of about PAIR_CHUNK pairs (a list of thousands of
    # pieces has tens of millions of pairs: their index arrays are not all held at once)
    blocks, held = [], 0
    for a, trips in enumerate(comp):
        if trips is None:
            continue
        k = len(trips)
        step = max(1, PAIR_CHUNK // k)
        for j0 in range(0, k, step):
            j1 = min(k, j0 + step)
            jj = np.repeat(np.arange(j0, j1), k); ii = np.tile(np.arange(k), j1 - j0)
            keep = ii != jj
            blocks.append((a, ii[keep], jj[keep])); held += int(keep.sum())
            if held >= PAIR_CHUNK:
                ask(blocks)
                blocks, held = [], 0
    if blocks:
        ask(blocks)
    return refuted


def _refuted_matrix(k, cols, segs):
    """refuted [k, k] bool of a list of k from the segments of `bits` of the pieces `cols` that left something undecided
    (segs[c]: the ceil(k / 32) words of piece cols[c]): column j = its unpacked bits; a piece that left nothing undecided
    is refuted by every other piece's member."""
    refuted = ~np.eye(k, dtype=bool)
    for j, seg in zip(cols, segs):
        refuted[:, j] = np.unpackbits(np.ascontiguousarray(seg, dtype="<u4").view(np.uint8), bitorder="little")[:k].astype(bool)
    return refuted


def _refuted_by_lists(comp, starts, engine, tol, groups, xrow, X_of, cat):
    """_refuted_by_members on an engine with `members_outside_lists` (REFUTE_ROUTE = "lists"): the lists themselves go up, once
    per level -- per member dimension a CSR of all lists (the rows of their pieces' members, sum of k integers) and the members'
    ok flags, left where interior_members wrote them -- then ONE call per pack of second pieces.  Only `undecided` comes to
    the host unconditionally: a list none of whose pieces left a pair undecided holds no subset and gets no matrix (None);
    for the others the segments of the pieces that left something undecided come down (_refuted_matrix).
    -> {list a: refuted [k, k] bool, or None = every pair refuted}."""
    dev = _on_device(engine)
    if dev:
        import torch
        up = lambda v: torch.as_tensor(v, device=f"cuda:{engine.device}")
    else:
        up = lambda v: v
    OK_of = {}
    for grp in groups:
        OK_of.setdefault(int(grp["x"].shape[1]), []).append(grp["ok"])
    OK_of = {d: cat(oks) for d, oks in OK_of.items()}
    # the lists of one member dimension, as a CSR over the rows of that dimension's X; every piece has a row (ok says
    # whether it holds a member), so no entry is -1
    alist = [a for a, trips in enumerate(comp) if trips is not None]
    klen = {a: len(comp[a]) for a in alist}
    nflat = sum(klen.values())
    list_a = np.zeros(nflat, np.int64)                      # the list of a flat piece
    for a in alist:
        list_a[starts[a]:starts[a] + klen[a]] = a
    csr, local = {}, {}
    for d in X_of:
        mine = [a for a in alist if comp[a][0][0].shape[1] == d]
        ptr = np.zeros(len(mine) + 1, np.int64)
        ptr[1:] = np.cumsum([klen[a] for a in mine])
        mem = np.concatenate([xrow[starts[a]:starts[a] + klen[a]] for a in mine]).astype(np.int32) if mine else np.zeros(0, np.int32)
        for n, a in enumerate(mine):
            local[a] = n
        csr[d] = (up(ptr.astype(np.int32)), up(mem))
    need = {}                                               # list a -> [(piece j of it, its words)] where something is undecided
    open_lists = set()
    for grp in groups:
        idx = np.asarray(grp["idx"], dtype=np.int64)
        Ac = grp["Ac"]
        d = int(Ac.shape[1])
        la = list_a[idx]
        kk = np.array([klen[a] for a in la.tolist()], np.int64)
        words = -(-kk // 32)
        wptr = np.zeros(len(idx) + 1, np.int64); wptr[1:] = np.cumsum(words)
        list_of = np.array([local[a] for a in la.tolist()], np.int32)
        self_pos = (idx - np.array([starts[a] for a in la.tolist()], np.int64)).astype(np.int32)
        bits, und = engine.members_outside_lists(Ac, grp["l"], grp["u"], X_of[d], OK_of[d], *csr[d], up(list_of), up(self_pos), up(wptr),
                                                 10 * tol)
        und = _to_host(und)
        hit = np.nonzero(und > 0)[0]
        if not len(hit):
            continue
        # only the segments of the pieces that left something undecided come down
        widx = np.concatenate([np.arange(wptr[p], wptr[p + 1]) for p in hit])
        if dev:
            got = bits.view(torch.int32)[torch.as_tensor(widx, device=bits.device)].cpu().numpy().view(np.uint32)
        else:
            got = np.asarray(bits)[widx]
        q0 = 0
        for p in hit.tolist():
            a = int(la[p])
            need.setdefault(a, []).append((int(self_pos[p]), got[q0:q0 + int(words[p])]))
            q0 += int(words[p])
            open_lists.add(a)
    refuted = {}
    for a in alist:
        if a not in open_lists:
            refuted[a] = None
            continue
        cols, segs = zip(*need[a])
        refuted[a] = _refuted_matrix(klen[a], cols, segs)
    return refuted


def remove_subsets_many(lists, engine, tol=1e-6, prefilter=True):
    """`remove_subsets` (src/sets.jl:889-902) for the solution graphs of ALL nodes of a level at once (src/algorithm.jl:84
    applies it to every node's S).  Every list is first brought down to the columns its pieces touch (a large net's pieces are
    local).  The reference asks k (k - 1) subset questions per list, each one LP per finite bound of the second polyhedron
    (src/sets.jl:376-407) -- 100 000 LPs for a node with 32 pieces.  Here a question is first put to ONE point: P1 ⊆ P2 needs
    every point of P1 in P2, so a member of P1 that violates a row of P2 by more than 10 tol settles "not a subset" without
    an LP (the reference's LP over P1 would come out below the bound by the same amount).  The member is a point of P1's
    relative interior (interior_members_batch: the slack LP of `exemplar`, src/sets.jl:591-642, over the inequality rows; one LP
    per piece, all pieces of the level in one batch) -- cells of a piecewise-affine solution map that merely touch are told
    apart by it -- and only the pairs it does not settle go to the LPs (issubset_batch, chunked).  An engine with
    `interior_members` and `members_outside` also puts the members to the pieces itself (_refuted_by_members).
    -> list of kept lists."""
    comp, jobs, where = [], [], []
    flat, starts = [], {}                                   # the pieces of all lists, one after the other; where list a starts
    for a, polys in enumerate(lists):
        k = len(polys) if polys is not None else 0
        if k < 2:
            comp.append(None)
            continue
        cols = np.unique(np.concatenate([P.support() for P in polys]))
        trips = [_triple((P.block(cols), P.l, P.u)) for P in polys]
        comp.append(trips)
        if prefilter:
            starts[a] = len(flat)
            flat += trips
    on_engine = bool(flat) and all(_has(engine, f) for f in ("interior_members", "members_outside"))
    refuted_of = _refuted_by_members(comp, flat, starts, engine, tol) if on_engine else {}
    member = interior_members_batch(flat, engine) if flat and not on_engine else []     # (no answer for a piece: its pairs go to the LPs)
    sub = {}
    for a, trips in enumerate(comp):
        if trips is None:
            continue
        k = len(trips)
        have = [i for i in range(k) if member and member[starts[a] + i] is not None]
        if a in refuted_of and refuted_of[a] is None:       # (the lists route: every pair of this list refuted, no matrix)
            sub[a] = None
            continue
        refuted = refuted_of.get(a, np.zeros((k, k), bool))  # refuted[i, j]: P1 = piece i has a member outside P2 = piece j
        if have:
            pts = np.stack([member[starts[a] + i] for i in have], axis=1)   # [d, members]
            for j in range(k):
                A2, l2, u2 = trips[j]
                ax = A2 @ pts[:A2.shape[1]]
                out = np.any(ax < (l2 - 10 * tol)[:, None], axis=0) | np.any(ax > (u2 + 10 * tol)[:, None], axis=0)
                refuted[have, j] = out
        sub[a] = np.zeros((k, k), bool)                     # (refuted pairs: not a subset)
        open_ = ~refuted
        np.fill_diagonal(open_, False)
        for i, j in np.argwhere(open_).tolist():
            jobs.append((trips[i], trips[j])); where.append((a, i, j))
    res = issubset_batch_chunked(jobs, engine, tol=tol) if jobs else []
    for (a, i, j), r in zip(where, res):
        sub[a][i, j] = bool(r)
    out = []
    for a, polys in enumerate(lists):
        if comp[a] is None:
            out.append(polys)
            continue
        if sub[a] is None:
            out.append(list(polys))
            continue
        k = len(polys)
        is_subset = np.zeros(k, bool)
        for i in range(k):
            if np.any(sub[a][i] & ~is_subset):              # (the diagonal is never set)
                is_subset[i] = True
        out.append([P for P, s_ in zip(polys, is_subset) if not s_])
    return out


# ---- the reference's own rules on the same solver: LPs as node-AVIs with Q = 0 --------------------------------------------
def _open(p, n):
    if hasattr(p, "open_bounds"):
        return p.open_bounds()
    return np.zeros(n, bool), np.zeros(n, bool)


def _solve_lps(cost, A, l, u, engine):
    """Batch of LPs  min cost_b' x  s.t.  l_b <= A_b x <= u_b  (B, m, d padded arrays) through the node solver.
    -> (status [B], x [B, d], lambda [B, m])."""
    d = A.shape[2]
    status, z = node_qp(None, cost, A, l, u, engine)
    return status, z[:, :d], z[:, d:]


def _isapprox(x, y, atol, rtol):
    """Julia's `isapprox(x, y; atol, rtol)` on vectors: norm(x - y) <= max(atol, rtol * max(norm(x), norm(y))) -- a condition on
    the 2-norm of the difference, not elementwise; when that norm is not finite (infinite entries), the component-wise scalar rule
    `a == b || (isfinite(a) && isfinite(b) && |a - b| <= max(atol, rtol * max(|a|, |b|)))` on every pair instead."""
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.linalg.norm(x - y)
        if np.isfinite(d):
            return bool(d <= max(atol, rtol * max(np.linalg.norm(x), np.linalg.norm(y))))
        fin = np.isfinite(x) & np.isfinite(y)
        close = np.abs(x - y) <= np.maximum(atol, rtol * np.maximum(np.abs(x), np.abs(y)))
        return bool(np.all((x == y) | (fin & close)))


def exemplar_slack_batch(polys, engine, tol=1e-2, slack_cap=1.0, strict=True, route=None):
    """`exemplar(poly; tol)` (src/sets.jl:591-642), the reference's own emptiness rule, for a batch:
        min eps  s.t.  A x + eps >= l,  -A x + eps >= -u                       (:608-619)
        eps > tol -> empty;  eps > -tol -> empty iff an OPEN bound is active (|dual| > tol), else a member;
        eps <= -tol -> a member with slack                                     (:625-641)
    plus the square-equality shortcut x = A \\ l (:599-606).  One LP per polyhedron in variables (x, eps), all in one call of
    the node solver.  eps is capped below at -slack_cap (an unbounded LP -- OSQP's status 4, which the reference does not
    handle -- means slack without end: a member either way).  -> (empty [B] bool, example list, eps [B]).
    route="polyhedron" on an engine with `exemplar_polys` (qpn_exemplar_polys): every item the shortcuts leave, closed or open,
    is ONE job of the batched simplex that expands its own slack LP and applies the rule to its own duals -- one call per shape,
    no node solve and no solve_lps call (_exemplar_slack_polyhedra); any other engine, and a shape beyond the kernel's limits,
    keeps today's route (route=None or "nodes").
    Parity unpinned: the reference holds no fixture for this rule; checked against HiGHS on seeded polyhedra and the hand-checked
    edge cases of tests/test_polyhedra.py (the norm-based `isapprox` of :599, the slack cap)."""
    if route not in (None, "nodes", "polyhedron"):
        raise ValueError(f"exemplar_slack_batch: unknown route {route!r}")
    Bn = len(polys)
    if Bn == 0:
        return np.zeros(0, bool), [], np.zeros(0)
    trips = [_triple(p) for p in polys]
    opens = [_open(p, len(t[1])) for p, t in zip(polys, trips)]
    empty = np.zeros(Bn, bool); eps_out = np.full(Bn, np.nan); example = [None] * Bn
    todo = []
    for b, ((A, l, u), (ol, oh)) in enumerate(zip(trips, opens)):
        n, d = A.shape
        if n == 0:
            empty[b] = False; continue                                                     # :594
        if n == d and not ol.any() and not oh.any() and _isapprox(l, u, tol, tol):             # :599-606
            try:
                x = np.linalg.solve(A, l)
                ok = _isapprox(A @ x, l, tol, tol)
            except np.linalg.LinAlgError:
                ok, x = False, None
            empty[b] = not ok; example[b] = x if ok else None
            continue
        todo.append(b)
    if todo and route == "polyhedron" and _has(engine, "exemplar_polys"):
        todo = _exemplar_slack_polyhedra(todo, trips, opens, engine, tol, slack_cap, strict, empty, example, eps_out)
    if todo and _has(engine, "solve_lps"):
        # closed polyhedra: the answer depends on eps alone -- the LP solver; with an open bound it depends on which duals the
        # solver returns: today's route
        closed = [b for b in todo if not opens[b][0].any() and not opens[b][1].any()]
        todo = [b for b in todo if opens[b][0].any() or opens[b][1].any()]
        _exemplar_slack_lps(closed, trips, engine, tol, slack_cap, strict, empty, example, eps_out)
    if todo:
        dmax = max(trips[b][0].shape[1] for b in todo) + 1
        mmax = max(2 * trips[b][0].shape[0] for b in todo) + 1
        A2, l2, _ = _padded([trips[b] for b in todo], mmax, dmax)                          # A x ... >= l; the rows are one-sided
        u2 = np.full((len(todo), mmax), INF)
        cost = np.zeros((len(todo), dmax)); cost[:, dmax - 1] = 1.0
        for k, b in enumerate(todo):
            A, l, u = trips[b]
            n, d = A.shape
            A2[k, :n, dmax - 1] = 1.0                                                      # A x + eps >= l
            A2[k, n:2 * n, :d] = -A; A2[k, n:2 * n, dmax - 1] = 1.0; l2[k, n:2 * n] = -u   # -A x + eps >= -u
            A2[k, mmax - 1, dmax - 1] = 1.0; l2[k, mmax - 1] = -slack_cap                  # eps >= -cap
        st, x, lam = _solve_lps(cost, A2, l2, u2, engine)
        for k, b in enumerate(todo):
            if st[k] != 1:
                if strict:
                    raise RuntimeError(f"exemplar_slack_batch: solver status {st[k]} on item {b}")
                continue                                    # (not strict: no answer for this item -- empty False, no example, eps nan)
            n, d = trips[b][0].shape
            eps = x[k, dmax - 1]; eps_out[b] = eps
            ol, oh = opens[b]
            if eps > tol:
                empty[b] = True
            elif eps > -tol:
                act_l = np.abs(lam[k, :n]) > tol; act_u = np.abs(lam[k, n:2 * n]) > tol    # :629-631
                empty[b] = bool(np.any(act_l & ol) or np.any(act_u & oh))
            if not empty[b]:
                example[b] = x[k, :d].copy()
    return empty, example, eps_out


def isempty_slack_batch(polys, engine, tol=1e-4, x=None, route=None):
    """`isempty(poly; tol, x)` (src/sets.jl:647-655) for a batch: membership of the given point first, else the exemplar rule
    (by `route`, see exemplar_slack_batch)."""
    out = np.zeros(len(polys), bool)
    inside = lambda p: x is not None and hasattr(p, "contains") and p.contains(np.asarray(x, dtype=np.float64))
    rest = [b for b, p in enumerate(polys) if not inside(p)]
    if rest:
        out[rest] = exemplar_slack_batch([polys[b] for b in rest], engine, tol=tol, route=route)[0]
    return out


def isempty_products(pieces, products, engine, tol=1e-4, points=None, point_of=None, point_tol=1e-6, slack_cap=1.0, strict=True):
    """The intersection tree's test of products of pieces (src/intersection.jl:66-105) for a batch, on an engine with
    `exemplar_products` (qpn_exemplar_products): a product is kept when its point lies in its closure (:74) and it is not empty
    (:83, `isempty` -> `exemplar`, the rule of exemplar_slack_batch).  pieces: [(A [r, d], l, u, open_lo, open_hi)], every distinct
    piece once, open flags on finite bounds only (Poly.open_bounds); products: tuples of positions in `pieces`, the factors in
    order, all of one product over the same d columns; points: the points (each of its products' d coordinates) and point_of: the
    point of each product -- both None: no closure test.
    The pieces go up once per d as one pool of rows, a product is the tuple of its factors' positions there, and the products are
    grouped by (d, n), n the number of their rows: one call per group, no copy of a piece per product.  The products
    exemplar_slack_batch answers without an LP (n == 0, the square-equality shortcut, :594-606) and the shapes beyond the kernel's
    limits (n > 511, d > 255, more than 32 factors) are stacked on the host, tested against their point there and go through
    exemplar_slack_batch(route="polyhedron").  A product that ends in EX_ITER_LIMIT or EX_FAILURE raises (strict; the lowest-numbered
    one is named) or stays unanswered.  -> (near [products] bool, empty [products] bool; a product that is not near is not asked)."""
    P = len(products)
    near = np.ones(P, bool); empty = np.zeros(P, bool)
    if P == 0:
        return near, empty
    rows_of = [p[0].shape[0] for p in pieces]
    any_open = [bool(p[3].any() or p[4].any()) for p in pieces]
    stacked = lambda t, c: np.concatenate([pieces[f][c] for f in products[t]])
    groups, host = {}, []
    for t, fs in enumerate(products):
        d = pieces[fs[0]][0].shape[1]
        n = sum(rows_of[f] for f in fs)
        shortcut = n == d and not any(any_open[f] for f in fs) and _isapprox(stacked(t, 1), stacked(t, 2), tol, tol)
        if n == 0 or shortcut or n > EX_MAX_N or d > EX_MAX_D or d < 1 or len(fs) > PROD_MAX_K:
            host.append(t)
        else:
            groups.setdefault(d, {}).setdefault(n, []).append(t)
    if host:
        polys = []
        for t in host:
            A = np.vstack([pieces[f][0] for f in products[t]]); l = stacked(t, 1); u = stacked(t, 2)
            if points is not None:
                ax = A @ np.asarray(points[point_of[t]], dtype=np.float64)
                near[t] = bool(np.all(l - point_tol <= ax) and np.all(ax - point_tol <= u))
            polys.append(_Flagged(A, l, u, stacked(t, 3), stacked(t, 4)))
        ask = [k for k, t in enumerate(host) if near[t]]
        if ask:
            empty[[host[k] for k in ask]] = exemplar_slack_batch([polys[k] for k in ask], engine, tol=tol, slack_cap=slack_cap, strict=strict,
                                                                 route="polyhedron")[0]
    failed = []
    for d in sorted(groups):
        used = sorted({f for ts in groups[d].values() for t in ts for f in products[t]})
        at = {f: i for i, f in enumerate(used)}
        A = np.vstack([pieces[f][0] for f in used]); l = np.concatenate([pieces[f][1] for f in used]); u = np.concatenate([pieces[f][2] for f in used])
        ol = np.concatenate([pieces[f][3] for f in used]).astype(np.uint8); oh = np.concatenate([pieces[f][4] for f in used]).astype(np.uint8)
        piece_row = np.concatenate([[0], np.cumsum([rows_of[f] for f in used])]).astype(np.int32)
        pts, pt_at = None, {}
        if points is not None:
            for ts in groups[d].values():
                for t in ts:
                    pt_at.setdefault(point_of[t], len(pt_at))
            pts = np.array([points[j] for j in pt_at], dtype=np.float64).reshape(len(pt_at), d)
        for n in sorted(groups[d]):
            ts = groups[d][n]
            k = max(len(products[t]) for t in ts)
            factors = np.full((len(ts), k), -1, np.int32)
            for i, t in enumerate(ts):
                factors[i, :len(products[t])] = [at[f] for f in products[t]]
            pof = None if pts is None else np.array([pt_at[point_of[t]] for t in ts], np.int32)
            res = engine.exemplar_products(A, l, u, ol, oh, piece_row, factors, n, point=pts, point_of=pof, point_tol=point_tol, tol=tol,
                                           slack_cap=slack_cap)
            nr = _to_host(res["near"]); em = _to_host(res["empty"]); how = _to_host(res["how"])
            near[ts] = nr != 0; empty[ts] = em != 0
            failed += [(t, int(h)) for t, h in zip(ts, how) if h in (EX_ITER_LIMIT, EX_FAILURE)]
    if failed and strict:
        t, how = min(failed)
        raise RuntimeError(f"isempty_products: exemplar status {how} on product {t}")
    return near, empty


TREE_ALIVE_GUESS = 64           # intersection_trees' first cap counts on at most this many live prefixes per tree and depth
TREE_FRONT_CAP = 1 << 20        # ... and it asks for no larger cap than this: the entry's workspace is about 16 cap L bytes


def intersection_trees(pieces, trees, engine, tol=1e-4, points=None, point_of=None, point_tol=1e-6, slack_cap=1.0, strict=True):
    """The intersection trees of `combine` (src/intersection.jl:66-105, :116-138) for a batch, on an engine with `intersection_trees`
    (qpn_intersection_trees): per tree the tuples -- one piece of every list -- whose point lies in the closure of every member and
    none of whose prefixes is empty, in the order `iterate` yields them; no tuple is formed on the host.  pieces: as
    isempty_products takes them; trees: [(lists, reds)], lists = L lists of positions in `pieces` (union t's pieces in the
    reference's order), reds = per list the number of its trailing members that are complement pieces (the redzone, :123): a tuple
    of complement pieces alone is no leaf.  points, point_of: the points and the point of each tree (both None: no closure test).
    A pool of rows goes up per d, the trees are grouped by (d, L): one call per group.  cap, the most tuples a depth may hold, starts
    as the largest over the depths of sum over the group's trees of min(prod_{s <= t} w_s, TREE_ALIVE_GUESS w_t) (w: the lists'
    widths); a call that overflows is made once more with the true products in place of the guess, and when those are beyond
    TREE_FRONT_CAP (the entry's workspace is about 16 cap L bytes: 48 MiB at this cap and L = 3) its trees fall back.  A tree goes to isempty_products (same pieces, all tuples) when the engine lacks the method, L
    is outside [2, 32], d is outside [1, 255], a piece of it has no rows, the longest pieces of its lists add up to more than 511
    rows, a piece of it is closed with isapprox(l, u) (a tuple of such pieces could take exemplar's square-equality shortcut,
    src/sets.jl:599-606, where the device runs the LP), or its group overflowed twice.  A candidate without an answer raises
    (strict), as isempty_products does.
    -> (leaves: per tree the list of tuples of positions in `pieces`, stats: dict(tested: the candidates tested on the tree route,
    products: the tuples the products route forms for those trees -- those of complement pieces alone are not counted --,
    fallback: the trees that took isempty_products, calls))."""
    T = len(trees)
    leaves = [None] * T
    stats = dict(tested=0, products=0, fallback=[], calls=0)
    rows_of = [p[0].shape[0] for p in pieces]
    flat = lambda p: not (p[3].any() or p[4].any()) and p[0].shape[0] > 0 and _isapprox(p[1], p[2], tol, tol)
    flat_of = {}
    groups = {}
    for g, (lists, reds) in enumerate(trees):
        L = len(lists)
        used = [f for mem in lists for f in mem]
        d = pieces[used[0]][0].shape[1] if used else 0
        for f in used:
            if f not in flat_of:
                flat_of[f] = flat(pieces[f])
        ok = _has(engine, "intersection_trees") and 2 <= L <= TREE_MAX_L and 1 <= d <= EX_MAX_D and all(rows_of[f] > 0 for f in used) and \
            sum(max((rows_of[f] for f in mem), default=0) for mem in lists) <= EX_MAX_N and not any(flat_of[f] for f in used)
        if ok:
            groups.setdefault((d, L), []).append(g)
        else:
            stats["fallback"].append(g)
    for (d, L) in sorted(groups):
        gs = groups[(d, L)]
        used = sorted({f for g in gs for mem in trees[g][0] for f in mem})
        at = {f: i for i, f in enumerate(used)}
        A = np.vstack([pieces[f][0] for f in used]); l = np.concatenate([pieces[f][1] for f in used]); u = np.concatenate([pieces[f][2] for f in used])
        ol = np.concatenate([pieces[f][3] for f in used]).astype(np.uint8); oh = np.concatenate([pieces[f][4] for f in used]).astype(np.uint8)
        piece_row = np.concatenate([[0], np.cumsum([rows_of[f] for f in used])]).astype(np.int32)
        list_mem = np.array([at[f] for g in gs for mem in trees[g][0] for f in mem], np.int32)
        widths = np.array([[len(mem) for mem in trees[g][0]] for g in gs], np.int64).reshape(len(gs), L)
        list_ptr = np.concatenate([[0], np.cumsum(widths.reshape(-1))]).astype(np.int32)
        list_red = np.array([trees[g][1] for g in gs], np.int32).reshape(-1)
        pts, pof = None, None
        if points is not None:
            pt_at = {}
            for g in gs:
                pt_at.setdefault(point_of[g], len(pt_at))
            pts = np.array([points[j] for j in pt_at], dtype=np.float64).reshape(len(pt_at), d)
            pof = np.array([pt_at[point_of[g]] for g in gs], np.int32)
        full = np.cumprod(widths.astype(object), axis=1)                        # (exact: Python integers)
        guess = np.minimum(full, TREE_ALIVE_GUESS * widths.astype(object))
        caps = [int(max(1, guess.sum(0).max())), int(max(1, full.sum(0).max()))]
        res = None
        for cap in ([caps[0]] if caps[0] >= caps[1] else caps):
            if cap > min(TREE_MAX_CAP, TREE_FRONT_CAP):
                break
            got = engine.intersection_trees(A, l, u, ol, oh, piece_row, L, list_ptr, list_mem, list_red, cap, point=pts, point_of=pof,
                                            point_tol=point_tol, tol=tol, slack_cap=slack_cap)
            stats["calls"] += 1
            if int(_to_host(got["overflow"])[0]) == 0:
                res = got
                break
        if res is None:
            stats["fallback"] += gs
            continue
        k = int(_to_host(res["n_leaves"])[0])
        tup = _to_host(res["leaves"])[:k]; owner = _to_host(res["leaf_tree"])[:k]
        if strict and int(_to_host(res["unanswered"]).sum()):
            raise RuntimeError(f"intersection_trees: {int(_to_host(res['unanswered']).sum())} candidates of the trees of (d, L) = ({d}, {L}) "
                               "ended without an answer")
        for g in gs:
            leaves[g] = []
        for row, o in zip(tup, owner):
            leaves[gs[int(o)]].append(tuple(used[int(f)] for f in row))
        stats["tested"] += int(_to_host(res["tested"]).sum())
        stats["products"] += int(full[:, -1].sum()) - sum(int(np.prod(np.array(trees[g][1], dtype=object))) for g in gs)
    back = sorted(stats["fallback"])
    stats["fallback"] = back
    if back:
        products, owner, pof = [], [], []
        for g in back:
            lists, reds = trees[g]
            comp = [[i >= len(mem) - r for i in range(len(mem))] for mem, r in zip(lists, reds)]
            for choice in itertools.product(*[list(zip(mem, c)) for mem, c in zip(lists, comp)]):
                if all(c for _, c in choice):
                    continue
                products.append(tuple(f for f, _ in choice)); owner.append(g)
                if points is not None:
                    pof.append(point_of[g])
        near, empty = isempty_products(pieces, products, engine, tol=tol, points=points, point_of=pof if points is not None else None,
                                       point_tol=point_tol, slack_cap=slack_cap, strict=strict) if products else ([], [])
        for g in back:
            leaves[g] = []
        for t, (fs, g) in enumerate(zip(products, owner)):
            if near[t] and not empty[t]:
                leaves[g].append(fs)
    return leaves, stats


class _Flagged:
    """A stacked product for exemplar_slack_batch: the triple and its open flags."""

    def __init__(self, A, l, u, open_lo, open_hi):
        self._t, self._o = (A, l, u), (np.asarray(open_lo, bool), np.asarray(open_hi, bool))

    def vectorize(self):
        return self._t

    def open_bounds(self):
        return self._o


def implicit_bounds_batch(polys, engine, tol=1e-4, route="jobs"):
    """`implicit_bounds(poly; tol)` (src/sets.jl:660-713) for a batch: which rows have implicitly equal lower and upper
    bounds on the polyhedron, and their values.  Per row that is not an explicit equality, the two LPs min / max a_i' x over
    the polyhedron (:676-706) -- ALL rows of ALL polyhedra in one call; an unbounded LP (RAY_TERM) gives -+inf as OSQP's
    status 4 does there.  An empty polyhedron raises "Empty set" like the reference (:688-690).
    route="polyhedron" on an engine with `implicit_bounds` (qpn_implicit_bounds): ONE job per polyhedron -- the crash and phase 1
    once, the rows' extremes from the basis the previous one left, a row whose values at two visited points differ by more than
    tol refuted without an LP -- one call per shape, no node solve and no solve_lps call (_implicit_bounds_polyhedra); any other
    engine, and a shape beyond the kernel's limits, keeps route="jobs".
    -> list of (implicitly_equality [n] bool, vals [n])."""
    if route not in ("jobs", "polyhedron"):
        raise ValueError(f"implicit_bounds_batch: unknown route {route!r}")
    trips = [_triple(p) for p in polys]
    if route == "polyhedron" and trips and _has(engine, "implicit_bounds"):
        return _implicit_bounds_polyhedra(trips, engine, tol)
    return _implicit_bounds_jobs(trips, engine, tol)


def _implicit_bounds_polyhedra(trips, engine, tol):
    """implicit_bounds_batch on an engine with `implicit_bounds`: the polyhedra packed by shape (rows, columns), one call per
    shape; an EMPTY polyhedron raises "Empty set" for the lowest-numbered one, any other status the error that names the
    polyhedron and the row whose solve ended it.  Shapes beyond the kernel's limits go the route of the jobs."""
    from .engine import colmajor
    packs, beyond = pack_by_shape(trips, beyond=lambda s: min(s) < 1 or s[0] > LP_MAX_R or s[1] > LP_MAX_D)
    out = [None] * len(trips)
    empty, failed = [], []
    for _, members, A, l, u in packs:
        res = engine.implicit_bounds(colmajor(A), l, u, tol=tol)
        st = _to_host(res["status"]); fr = _to_host(res["fail_row"]); eq = _to_host(res["eq"]).astype(bool); vals = _to_host(res["vals"])
        for t, b in enumerate(members):
            if st[t] == IB_EMPTY:
                empty.append(b)
            elif st[t] != IB_OK:
                failed.append((b, int(st[t]), int(fr[t])))
            out[b] = (eq[t].copy(), vals[t].copy())
    # (the emptiness of the shapes beyond the limits is asked before anything is raised: the lowest-numbered empty one is named)
    empt = isempty_batch([trips[b] for b in beyond], engine) if beyond else np.zeros(0, bool)
    empty += [b for b, e in zip(beyond, empt) if e]
    if empty:
        raise RuntimeError(f"Empty set (polyhedron {min(empty)})")
    if failed:
        b, st, row = min(failed)
        raise RuntimeError(f"implicit_bounds_batch: status {st} on polyhedron {b}, row {row}")
    if beyond:
        for b, got in zip(beyond, _implicit_bounds_jobs([trips[b] for b in beyond], engine, tol, names=beyond, empt=empt)):
            out[b] = got
    return out


def irredundant_batch(polys, engine, tol=1e-8):
    """The polyhedra without the bounds their other bounds imply (qpn_irredundant_bounds; irredundant_bounds_host states the
    method): what the reference's `project` (src/sets.jl:501-523) gives a projected piece by going through its vertices.  The
    polyhedra packed by shape (rows, columns), one call per shape; a Poly in local form goes up over its own columns.
    -> a list of the same length and order: a Poly with the removed bounds at -+inf, a row with both bounds gone dropped, the
    order of the rows and the open flags of the bounds that stay kept.  An item comes back as it was given -- the same object --
    when nothing of it is removed, when its shape is beyond the kernel's limits, when the engine has no `irredundant_bounds`, and
    when its status is not OK; that includes EMPTY: emptiness is `combine`'s business.  There is no other route."""
    from .engine import colmajor
    from .programs import Poly
    polys = list(polys)
    if not polys or not _has(engine, "irredundant_bounds"):
        return polys
    trips = [_triple((p.local()[1], p.l, p.u) if hasattr(p, "local") else p) for p in polys]
    packs, _ = pack_by_shape(trips, beyond=lambda s: min(s) < 1 or s[0] > LP_MAX_R or s[1] > LP_MAX_D)
    out = list(polys)
    for _, members, A, l, u in packs:
        res = engine.irredundant_bounds(colmajor(A), l, u, tol=tol)
        st = _to_host(res["status"]); lr = _to_host(res["lr"]); ur = _to_host(res["ur"])
        for t, b in enumerate(members):
            if st[t] != IB_OK or (np.array_equal(lr[t], l[t]) and np.array_equal(ur[t], u[t])):
                continue
            keep = np.isfinite(lr[t]) | np.isfinite(ur[t])
            p = polys[b]
            olo, ohi = _open(p, len(keep))
            olo = (olo & np.isfinite(lr[t]))[keep]; ohi = (ohi & np.isfinite(ur[t]))[keep]
            if getattr(p, "_cols", None) is not None:
                cols, Al = p.local()
                out[b] = Poly.from_local(p.ncols, cols, Al[keep], lr[t][keep], ur[t][keep], normalise=False, open_lo=olo, open_hi=ohi)
            else:
                Ad = np.atleast_2d(np.asarray(p.vectorize()[0] if hasattr(p, "vectorize") else p[0], dtype=np.float64))
                out[b] = Poly(Ad[keep], lr[t][keep], ur[t][keep], normalise=False, open_lo=olo, open_hi=ohi)
    return out


def _implicit_bounds_jobs(trips, engine, tol, names=None, empt=None):
    """implicit_bounds_batch's route of the jobs: the emptiness projection on the node solver (empt: its answer, when the caller
    has it), then two LPs per row that is not an explicit equality.  names: the polyhedra's numbers in the caller's list (error
    messages)."""
    nm = (lambda b: b) if names is None else (lambda b: names[b])
    if empt is None:
        empt = isempty_batch(trips, engine) if trips else np.zeros(0, bool)
    if empt.any():
        raise RuntimeError(f"Empty set (polyhedron {nm(int(np.nonzero(empt)[0][0]))})")
    jobs = []                                                   # (poly, row, sign)
    out = []
    for b, (A, l, u) in enumerate(trips):
        n = A.shape[0]
        eq = np.zeros(n, bool); vals = np.full(n, INF)
        for i in range(n - 1, -1, -1):                          # (the reference walks the rows from the last, :670)
            if np.isclose(l[i], u[i], rtol=0, atol=tol) or (l[i] == u[i]):
                eq[i] = True; vals[i] = 0.5 * (l[i] + u[i])
            else:
                jobs.append((b, i, 1.0)); jobs.append((b, i, -1.0))
        out.append([eq, vals])
    if jobs and _has(engine, "solve_lps"):
        ext = _row_extremes_lps(trips, jobs, engine, nm)
        jobs = []
        _implicit_from_extremes(trips, out, ext, tol)
    if jobs:
        dmax = max(trips[b][0].shape[1] for b, _, _ in jobs); mmax = max(trips[b][0].shape[0] for b, _, _ in jobs)
        A2, l2, u2 = _padded([trips[b] for b, _, _ in jobs], mmax, dmax)
        cost = np.zeros((len(jobs), dmax))
        big = np.zeros(len(jobs))
        for k, (b, i, sg) in enumerate(jobs):
            A, l, u = trips[b]
            cost[k, :A.shape[1]] = sg * A[i]
            # The objective IS row i, so the LP is unbounded only through that row's own open side.  The pivoting method does
            # not always end an unbounded degenerate LP in a ray (it may stop at a point its own post-check then rejects), so
            # that side is closed far out and an optimum AT the far bound is read as "unbounded" (the reference reads OSQP's
            # dual-infeasible status the same way, :691-693, :704-706).
            fin = np.concatenate([l[np.isfinite(l)], u[np.isfinite(u)], [1.0]])
            big[k] = 1e6 * max(1.0, float(np.max(np.abs(fin))))
            if sg > 0 and l[i] == -INF:
                l2[k, i] = -big[k]
            if sg < 0 and u[i] == INF:
                u2[k, i] = big[k]
        st, x, _ = _solve_lps(cost, A2, l2, u2, engine)
        val = [float(trips[b][0][i] @ x[k, :trips[b][0].shape[1]]) if st[k] == 1 else np.nan for k, (b, i, sg) in enumerate(jobs)]
        # an optimum AT the far bound is read as "unbounded" only if it follows the bound: those LPs are solved once more with the
        # bound ten times as far out -- an unbounded row's optimum moves with it, a bounded row whose extreme merely lies beyond
        # 1e6 x the scale keeps its value (and is reported as the finite number it is)
        def closed_here(k):                                 # was this job's open side closed artificially?
            b, i, sg = jobs[k]
            return (sg > 0 and trips[b][1][i] == -INF) or (sg < 0 and trips[b][2][i] == INF)
        # (a row whose whole range lies beyond the far bound makes the closed LP infeasible -- RAY_TERM -- although the set is
        #  not empty: such jobs are looked at again too)
        again = [k for k in range(len(jobs)) if (st[k] == 1 and abs(val[k]) >= big[k] * (1.0 - 1e-6)) or (st[k] == 2 and closed_here(k))]
        if again:
            l3 = l2[again].copy(); u3 = u2[again].copy()
            for t, k in enumerate(again):
                b, i, sg = jobs[k]
                if sg > 0: l3[t, i] = -10.0 * big[k]
                else: u3[t, i] = 10.0 * big[k]
            st3, x3, _ = _solve_lps(cost[again], A2[again], l3, u3, engine)
            for t, k in enumerate(again):
                b, i, sg = jobs[k]
                if st3[t] == 1:
                    v3 = float(trips[b][0][i] @ x3[t, :trips[b][0].shape[1]])
                    if abs(v3) < 10.0 * big[k] * (1.0 - 1e-6):
                        val[k] = v3; big[k] = INF; st[k] = 1     # bounded after all
                    else:
                        big[k] = 0.0; val[k] = 0.0; st[k] = 1    # follows the bound: unbounded
                elif st3[t] == 2:
                    big[k] = 0.0; val[k] = 0.0; st[k] = 1        # still out of reach ten times further out: read as unbounded
        ext = {}
        for k, (b, i, sg) in enumerate(jobs):
            if st[k] == 1:
                v = val[k]
                if abs(v) >= big[k] * (1.0 - 1e-6):
                    v = -INF if sg > 0 else INF                 # at the far bound: unbounded in that direction
            elif st[k] == 2:
                v = -INF if sg > 0 else INF                     # unbounded in that direction (:691-693, :704-706)
            else:
                raise RuntimeError(f"implicit_bounds_batch: solver status {st[k]} on polyhedron {nm(b)}, row {i}")
            ext[(b, i, sg)] = v
        _implicit_from_extremes(trips, out, ext, tol)
    return [(eq, vals) for eq, vals in out]


def _implicit_from_extremes(trips, out, ext, tol):
    """implicit_bounds_batch's last step: rows whose minimum and maximum over the polyhedron coincide (ext[(b, i, +-1.0)])."""
    for b, (A, l, u) in enumerate(trips):
        eq, vals = out[b]
        for i in range(A.shape[0]):
            if (b, i, 1.0) in ext:
                lo_, hi_ = ext[(b, i, 1.0)], ext[(b, i, -1.0)]
                eq[i] = bool(np.isfinite(lo_) and np.isfinite(hi_) and abs(lo_ - hi_) <= tol)
                if eq[i]:
                    vals[i] = 0.5 * (hi_ + lo_)


def _row_extremes_lps(trips, jobs, engine, nm=lambda b: b):
    """implicit_bounds_batch's LPs on an engine with `solve_lps`: the polyhedra that have jobs are packed by shape (rows,
    columns) and go up once per pack; a job names its objective by (row, sign), so no cost vector and no copy of the
    polyhedron is made for it; an unbounded row is the solver's own answer.  jobs: [(polyhedron, row, sign)].
    -> {(b, i, sign): the extreme of a_i'x, -+inf when unbounded}."""
    from .engine import colmajor
    of, ext = {}, {}
    for b, i, sg in jobs:
        of.setdefault(b, []).append((i, sg))
    for _, members, A, l, u in pack_by_shape(trips, sorted(of))[0]:
        keys = [(b, i, sg) for b in members for i, sg in of[b]]
        poly_of = np.repeat(np.arange(len(members), dtype=np.int32), [len(of[b]) for b in members])
        res = engine.solve_lps(colmajor(A), l, u, poly_of, obj_row=np.array([k[1] for k in keys], np.int32),
                               obj_sign=np.array([int(k[2]) for k in keys], np.int32))
        st = _to_host(res["status"]); obj = _to_host(res["obj"])
        for t, (b, i, sg) in enumerate(keys):
            if st[t] == LP_OPTIMAL:
                ext[(b, i, sg)] = float(sg * obj[t])
            elif st[t] == LP_UNBOUNDED:
                ext[(b, i, sg)] = -INF if sg > 0 else INF       # (:691-693, :704-706)
            else:
                raise RuntimeError(f"implicit_bounds_batch: LP status {st[t]} on polyhedron {nm(b)}, row {i}")
    return ext


def _exemplar_slack_lps(items, trips, engine, tol, slack_cap, strict, empty, example, eps_out):
    """exemplar_slack_batch's slack LPs of closed polyhedra on an engine with `solve_lps`, packed by shape: rows [A, 1] >= l,
    [-A, 1] >= -u and eps >= -cap; the objective eps is the last row itself.  Fills empty, example, eps_out at `items`."""
    from .engine import colmajor
    for (n, d), members, A, l, u in pack_by_shape(trips, items)[0]:
        k = len(members)
        A2, l2, u2 = exemplar_rows(A, l, u, slack_cap)
        res = engine.solve_lps(colmajor(A2), l2, u2, np.arange(k, dtype=np.int32),
                               obj_row=np.full(k, 2 * n, np.int32), obj_sign=np.ones(k, np.int32))
        st = _to_host(res["status"]); x = _to_host(res["x"])
        for t, b in enumerate(members):
            if st[t] != LP_OPTIMAL:
                if strict:
                    raise RuntimeError(f"exemplar_slack_batch: LP status {st[t]} on item {b}")
                continue
            eps_out[b] = x[t, d]
            empty[b] = bool(x[t, d] > tol)
            if not empty[b]:
                example[b] = x[t, :d].copy()


def _exemplar_slack_polyhedra(items, trips, opens, engine, tol, slack_cap, strict, empty, example, eps_out):
    """exemplar_slack_batch on an engine with `exemplar_polys`: the items packed by shape (rows, columns), one call per shape; the
    engine expands the slack LPs and applies the rule, open bounds included.  Fills empty, example, eps_out at `items`; an item
    that ends in EX_ITER_LIMIT or EX_FAILURE raises (strict; the lowest-numbered one is named) or stays unanswered.
    -> the items whose shape is beyond the kernel's limits (they take today's route)."""
    from .engine import colmajor
    packs, beyond = pack_by_shape(trips, items, extras=([o[0] for o in opens], [o[1] for o in opens]),
                                  beyond=lambda s: min(s) < 1 or s[0] > EX_MAX_N or s[1] > EX_MAX_D)
    failed = []
    for _, members, A, l, u, ol, oh in packs:
        res = engine.exemplar_polys(colmajor(A), l, u, ol.astype(np.uint8), oh.astype(np.uint8), tol=tol, slack_cap=slack_cap)
        em = _to_host(res["empty"]); how = _to_host(res["how"]); eps = _to_host(res["eps"]); x = _to_host(res["x"])
        for t, b in enumerate(members):
            if how[t] in (EX_ITER_LIMIT, EX_FAILURE):
                failed.append((b, int(how[t])))
                continue                                    # (not strict: no answer for this item -- empty False, no example, eps nan)
            eps_out[b] = eps[t]
            empty[b] = bool(em[t])
            if not empty[b]:
                example[b] = x[t].copy()
    if failed and strict:
        b, how = min(failed)
        raise RuntimeError(f"exemplar_slack_batch: exemplar status {how} on item {b}")
    return beyond
