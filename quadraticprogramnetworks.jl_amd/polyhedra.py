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
reference's rule to its own duals (exemplar_polys_host is the twin).
"""
from __future__ import annotations

import numpy as np

INF = np.inf


def exemplar_batch(polys, engine):
    """-> (empty [B] bool, example [B] list of x or None, status [B] int32).

    `polys`: sequence of objects with `vectorize() -> (A, l, u)` (programs.Poly) or (A, l, u) triples.
    `engine`: anything with `solve_nodes` (the HIP engine: fused assembly + solve) or `solve_avi_batch`."""
    trip = [p.vectorize() if hasattr(p, "vectorize") else p for p in polys]
    B = len(trip)
    if B == 0:
        return np.zeros(0, bool), [], np.zeros(0, np.int32)
    dims = [np.atleast_2d(t[0]).shape for t in trip]
    d = max(1, max(s[1] for s in dims))
    m = max(1, max(s[0] for s in dims))
    A = np.zeros((B, m, d)); l = np.full((B, m), -INF); u = np.full((B, m), INF)
    for b, (Ab, lb, ub) in enumerate(trip):
        Ab = np.atleast_2d(np.asarray(Ab, dtype=np.float64))
        r, c = Ab.shape
        A[b, :r, :c] = Ab
        l[b, :r] = np.asarray(lb, dtype=np.float64); u[b, :r] = np.asarray(ub, dtype=np.float64)
    Q = np.broadcast_to(np.eye(d), (B, d, d)).copy()
    qd = np.zeros((B, d))
    if hasattr(engine, "solve_nodes"):
        from .engine import colmajor
        res = engine.solve_nodes(colmajor(Q), np.zeros((B, d, 1)), qd, colmajor(A), np.zeros((B, m, 1)), l, u, np.zeros(1))
    else:
        M = np.zeros((B, d + m, d + m))
        M[:, :d, :d] = Q; M[:, :d, d:] = -np.swapaxes(A, 1, 2); M[:, d:, :d] = A
        lo = np.concatenate([np.full((B, d), -INF), l], axis=1); hi = np.concatenate([np.full((B, d), INF), u], axis=1)
        kind = np.concatenate([np.zeros((B, d), np.uint8), np.ones((B, m), np.uint8)], axis=1)
        res = engine.solve_avi_batch(np.swapaxes(M, 1, 2), np.zeros((B, d + m)), lo, hi, kind=kind)
    status = np.asarray(res["status"]).astype(np.int32)
    z = np.asarray(res["z"])
    empty = status != 1
    example = [None if empty[b] else z[b, : dims[b][1]].copy() for b in range(B)]
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
    if len(pairs) and _has_subset_pairs(engine):
        return _issubset_pairs_route(pairs, engine, tol)
    queries, owner = [], []
    keyed = {}                                   # per polyhedron (the same object shows up in many pairs): its rows as hashable keys

    def rows_of(P):
        got = keyed.get(id(P))
        if got is None:
            A, l, u = (P.vectorize() if hasattr(P, "vectorize") else P)
            A = np.atleast_2d(np.asarray(A, dtype=np.float64))
            Ar = np.round(A, 9) + 0.0
            got = keyed[id(P)] = (A, np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64), [Ar[r].tobytes() for r in range(A.shape[0])], P)
        return got

    for k, (P1, P2) in enumerate(pairs):
        A1, l1, u1, k1, _ = rows_of(P1)
        A2, l2, u2, k2, _ = rows_of(P2)
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


def _has_subset_pairs(engine):
    return callable(getattr(engine, "issubset_pairs", None))


def _subset_packs(pairs):
    """The calls of issubset_pairs that answer `pairs`: the distinct polyhedra (by id: the same object shows up in many pairs) are
    packed by shape (rows, columns), first and second pieces apart, and every pair of shapes is one call with its index arrays
    into the two packs.  -> ([(positions in pairs, (A1c, l1, u1, A2c, l2, u2, pi, pj))], positions beyond the kernel's limits)."""
    from .engine import colmajor
    trips = {}

    def trip_of(P):
        got = trips.get(id(P))
        if got is None:
            A, l, u = (P.vectorize() if hasattr(P, "vectorize") else P)
            A = np.atleast_2d(np.asarray(A, dtype=np.float64))
            got = trips[id(P)] = (A, np.asarray(l, dtype=np.float64).reshape(A.shape[0]), np.asarray(u, dtype=np.float64).reshape(A.shape[0]), P)
        return got

    groups, beyond = {}, []
    for k, (P1, P2) in enumerate(pairs):
        A1, A2 = trip_of(P1)[0], trip_of(P2)[0]
        if A1.shape[1] != A2.shape[1]:
            raise ValueError(f"issubset_batch: pair {k} has polyhedra in {A1.shape[1]} and {A2.shape[1]} variables")
        if max(A1.shape[0], A2.shape[0]) > LP_MAX_R or A1.shape[1] > LP_MAX_D or min(A1.shape + A2.shape) < 1:
            beyond.append(k)
        else:
            groups.setdefault((A1.shape, A2.shape), []).append(k)
    calls = []
    for ((r1, d), (r2, _)), ks in sorted(groups.items()):
        packs = ({}, {})                                     # id -> position, first and second pieces
        idx = np.empty((2, len(ks)), np.int32)
        for t, k in enumerate(ks):
            for side in (0, 1):
                idx[side, t] = packs[side].setdefault(id(pairs[k][side]), len(packs[side]))
        arrs = []
        for side, r in ((0, r1), (1, r2)):
            members = [trips[i] for i in packs[side]]        # (insertion order = position)
            arrs += [colmajor(np.stack([m[0] for m in members]).reshape(len(members), r, d)),
                     np.stack([m[1] for m in members]), np.stack([m[2] for m in members])]
        calls.append((ks, tuple(arrs) + (idx[0].copy(), idx[1].copy())))
    return calls, beyond


def _issubset_pairs_route(pairs, engine, tol):
    """issubset_batch on an engine with `issubset_pairs`: one call per pair of shapes (_subset_packs), `sub` is the answer.  A
    shape beyond the kernel's limits keeps the route of the emptiness queries."""
    calls, beyond = _subset_packs(pairs)
    out = np.ones(len(pairs), bool)
    for ks, args in calls:
        out[ks] = _to_host(engine.issubset_pairs(*args, tol=tol)["sub"]).astype(bool)
    if beyond:
        out[beyond] = issubset_batch([pairs[k] for k in beyond], _WithoutSubsetPairs(engine), tol=tol)
    return out


class _WithoutSubsetPairs:
    """The engine without issubset_pairs: issubset_batch builds its emptiness queries."""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        if name == "issubset_pairs":
            raise AttributeError(name)
        return getattr(self._eng, name)


LP_CHUNK_BYTES = 1 << 30          # padded input of one batched LP call (host arrays; the device copy is as large again)


def issubset_batch_chunked(pairs, engine, tol=1e-6, chunk_bytes=None):
    """issubset_batch with the batch cut into calls whose padded host arrays stay below chunk_bytes (a level of a large net
    asks millions of subset questions; one call for all of them would need their padded copies all at once).  On an engine with
    `issubset_pairs` a call's arrays are the packs of its distinct polyhedra and two indices per pair: those bytes are counted."""
    chunk_bytes = chunk_bytes or LP_CHUNK_BYTES
    out = np.ones(len(pairs), bool)
    packed = _has_subset_pairs(engine)                       # that route uploads every distinct polyhedron of a call once
    start = 0
    while start < len(pairs):
        cost, stop, seen = 0, start, set()
        while stop < len(pairs):
            (A1, l1, _), (A2, l2, u2) = [(_trip(P)) for P in pairs[stop]]
            rows1, d = np.atleast_2d(A1).shape
            if packed:
                c = 8                                        # its two indices; a polyhedron counts where it first shows up
                for side, (P, A) in enumerate(zip(pairs[stop], (A1, A2))):
                    if (side, id(P)) not in seen:
                        c += (np.size(A) + 2 * np.atleast_2d(A).shape[0]) * 8
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


def interior_member_counts(l, u):
    """The slot counts (ne, nlo, nhi) of a batch's interior-member records: the largest number of equality rows (finite l == u),
    of other rows with a finite lower bound and of other rows with a finite upper bound of any item.  l, u [B, r]."""
    l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    eq = np.isfinite(l) & (l == u)
    lo = ~eq & np.isfinite(l); hi = ~eq & np.isfinite(u)
    return int(eq.sum(1).max(initial=0)), int(lo.sum(1).max(initial=0)), int(hi.sum(1).max(initial=0))


def interior_member_records(A, l, u, delta):
    """The node records of the interior-member queries of B polyhedra of one size, A [B, r, d] (math layout), l, u [B, r], packed
    straight into the ABI's column-major blocks -> (Qc [B, nf, nf], qd [B, nf], Ac [B, nf, mp], ll, uu [B, mp]) with
    nf = d + 1 + ne, mp = max(16, nlo + nhi rounded up to 16), (ne, nlo, nhi) = interior_member_counts(l, u); p = 1, R = 0, B = 0.
    The counts of equality / lower / upper rows differ from piece to piece: the free block is padded with idle multipliers (a unit
    diagonal entry, no coupling: mu = 0) and the rows with inert ones (0'z in (-inf, inf)) up to the batch's largest.
    This is the numpy twin of Engine.assemble_interior_nodes (qpn_assemble_interior_nodes), and the route of engines without it."""
    A = np.asarray(A, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    B, r, d = A.shape
    eq = np.isfinite(l) & (l == u)
    lo = ~eq & np.isfinite(l); hi = ~eq & np.isfinite(u)
    ne, nlo, nhi = int(eq.sum(1).max(initial=0)), int(lo.sum(1).max(initial=0)), int(hi.sum(1).max(initial=0))

    def pick(mask, cnt):                                  # first `cnt` row indices with the mask set, ascending; valid flags
        order = np.argsort(~mask, axis=1, kind="stable")[:, :cnt]
        return order, np.take_along_axis(mask, order, axis=1)

    (E, Ev), (LO, LOv), (HI, HIv) = pick(eq, ne), pick(lo, nlo), pick(hi, nhi)
    bidx = np.arange(B)[:, None]
    rows_of = lambda sel, valid: A[bidx, sel] * valid[:, :, None]        # (whole rows by index pairs: no index broadcast over d)
    nf = d + 1 + ne                                       # free block: [x; eps; mu_E]
    mi = nlo + nhi
    mp = max(16, -(-mi // 16) * 16)
    Qc = np.zeros((B, nf, nf)); qd = np.zeros((B, nf)); Ac = np.zeros((B, nf, mp))
    ll = np.full((B, mp), -INF); uu = np.full((B, mp), INF)
    ar = np.arange(d + 1)
    Qc[:, ar, ar] = delta
    qd[:, d] = 1.0
    if ne:
        AE = rows_of(E, Ev)                               # [B, ne, d], zero rows in the idle slots
        # math layout: Qd' = [[delta I, -A_E'], [A_E, 0]] (eps column of A_E is 0); Qc is its transpose per item
        Qc[:, d + 1:, :d] = -AE
        Qc[:, :d, d + 1:] = np.swapaxes(AE, 1, 2)
        je = d + 1 + np.arange(ne)
        Qc[:, je, je] = np.where(Ev, 0.0, 1.0)            # idle multipliers: 1 * mu = 0
        qd[:, d + 1:] = np.where(Ev, -np.take_along_axis(l, E, axis=1), 0.0)
    if nlo:
        Ac[:, :d, :nlo] = np.swapaxes(rows_of(LO, LOv), 1, 2); Ac[:, d, :nlo] = np.where(LOv, 1.0, 0.0)
        ll[:, :nlo] = np.where(LOv, np.take_along_axis(l, LO, axis=1), -INF)
    if nhi:
        Ac[:, :d, nlo:mi] = np.swapaxes(rows_of(HI, HIv), 1, 2); Ac[:, d, nlo:mi] = np.where(HIv, -1.0, 0.0)
        uu[:, nlo:mi] = np.where(HIv, np.take_along_axis(u, HI, axis=1), INF)
    return Qc, qd, Ac, ll, uu


def members_outside_host(Ajc, lj, uj, X, pi, pj, t):
    """The numpy twin of Engine.members_outside (qpn_members_outside), same operations in the same order: out [pairs] uint8, 1 where
    member X[pi[q]] violates a row of piece pj[q] -- a.x < l - t or a.x > u + t -- with a.x summed over ascending columns,
    acc = acc + a * x[c].  Ajc [Bj, d, rj] (the pieces' matrices in the ABI layout), lj, uj [Bj, rj], X [Bi, d]."""
    Ajc = np.asarray(Ajc, dtype=np.float64); lj = np.asarray(lj, dtype=np.float64); uj = np.asarray(uj, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64); pi = np.asarray(pi, dtype=np.int64); pj = np.asarray(pj, dtype=np.int64)
    Bj, d, rj = Ajc.shape
    out = np.zeros(len(pi), np.uint8)
    step = max(1, (1 << 24) // max(1, rj))                # (pairs x rows doubles per slice)
    for s in range(0, len(pi), step):
        qi, qj = pi[s:s + step], pj[s:s + step]
        acc = np.zeros((len(qi), rj))
        for c in range(d):
            acc = acc + Ajc[qj, c, :] * X[qi, c][:, None]
        with np.errstate(invalid="ignore"):
            out[s:s + step] = np.any((acc < lj[qj] - t) | (acc > uj[qj] + t), axis=1)
    return out


PAIR_CHUNK = 1 << 22             # (member, piece) pairs of one members_outside call of remove_subsets_many, about


def _on_device(engine):
    return getattr(engine, "device", -1) >= 0


def _interior_member_groups(trips, engine, delta=1e-2, chunk=20000):
    """interior_members_batch's work: the queries packed by size (rows, columns), one engine call per pack of at most `chunk`.
    -> list of dict(idx: positions in `trips`, x [B, d], ok [B], and with an engine that has interior_members also Ac [B, d, r],
    l, u [B, r]: the pack as the engine got it).  x and ok stay where the engine left them (device tensors on a device engine)."""
    groups = {}
    prepared = []
    for i, (A, l, u) in enumerate(trips):
        A = np.atleast_2d(np.asarray(A, dtype=np.float64))
        l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
        prepared.append((A, l, u))
        groups.setdefault((A.shape[0], A.shape[1]), []).append(i)
    fused = callable(getattr(engine, "interior_members", None))
    out = []
    for (r, d), idx_all in sorted(groups.items()):
        for c0 in range(0, len(idx_all), chunk):
            idx = idx_all[c0:c0 + chunk]
            B = len(idx)
            A = np.stack([prepared[i][0] for i in idx]).reshape(B, r, d)
            l = np.stack([prepared[i][1] for i in idx]).reshape(B, r); u = np.stack([prepared[i][2] for i in idx]).reshape(B, r)
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
        ok_h[idx] = _to_host(grp["ok"]).astype(bool)
        X_of.setdefault(d, []).append(grp["x"])
    dev = _on_device(engine)
    if dev:
        import torch
    cat = (lambda xs: xs[0] if len(xs) == 1 else torch.cat(xs)) if dev else (lambda xs: xs[0] if len(xs) == 1 else np.concatenate(xs))
    X_of = {d: cat(xs) for d, xs in X_of.items()}
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
    flat, flat_of, starts = [], [], {}
    for a, polys in enumerate(lists):
        k = len(polys) if polys is not None else 0
        if k < 2:
            comp.append(None)
            continue
        cols = np.unique(np.concatenate([P.support() for P in polys]))
        trips = [(P.block(cols), P.l, P.u) for P in polys]
        comp.append(trips)
        if prefilter:
            starts[a] = len(flat)
            flat += trips; flat_of += [(a, i) for i in range(k)]
    on_engine = bool(flat) and all(callable(getattr(engine, f, None)) for f in ("interior_members", "members_outside"))
    refuted_of = _refuted_by_members(comp, flat, starts, engine, tol) if on_engine else {}
    member = {}
    if flat and not on_engine:
        for key, pt in zip(flat_of, interior_members_batch(flat, engine)):      # (no answer for a piece: its pairs go to the LPs)
            member[key] = pt
    sub = {}
    for a, trips in enumerate(comp):
        if trips is None:
            continue
        k = len(trips)
        have = [i for i in range(k) if member.get((a, i)) is not None]
        refuted = refuted_of.get(a, np.zeros((k, k), bool))  # refuted[i, j]: P1 = piece i has a member outside P2 = piece j
        if have:
            pts = np.stack([member[(a, i)] for i in have], axis=1)          # [d, members]
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
        k = len(polys)
        is_subset = np.zeros(k, bool)
        for i in range(k):
            if np.any(sub[a][i] & ~is_subset):              # (the diagonal is never set)
                is_subset[i] = True
        out.append([P for P, s_ in zip(polys, is_subset) if not s_])
    return out


# ---- the reference's own rules on the same solver: LPs as node-AVIs with Q = 0 --------------------------------------------
def _trip(p):
    return p.vectorize() if hasattr(p, "vectorize") else p


def _open(p, n):
    if hasattr(p, "open_bounds"):
        return p.open_bounds()
    return np.zeros(n, bool), np.zeros(n, bool)


def _solve_lps(cost, A, l, u, engine):
    """Batch of LPs  min cost_b' x  s.t.  l_b <= A_b x <= u_b  (B, m, d padded arrays) through the node solver.
    -> (status [B], x [B, d], lambda [B, m])."""
    B, m, d = A.shape
    if hasattr(engine, "solve_nodes"):
        from .engine import colmajor
        res = engine.solve_nodes(colmajor(np.zeros((B, d, d))), np.zeros((B, d, 1)), cost, colmajor(A), np.zeros((B, m, 1)), l, u,
                                 np.zeros(1))
    else:
        M = np.zeros((B, d + m, d + m))
        M[:, :d, d:] = -np.swapaxes(A, 1, 2); M[:, d:, :d] = A
        lo = np.concatenate([np.full((B, d), -INF), l], axis=1); hi = np.concatenate([np.full((B, d), INF), u], axis=1)
        kind = np.concatenate([np.zeros((B, d), np.uint8), np.ones((B, m), np.uint8)], axis=1)
        res = engine.solve_avi_batch(np.swapaxes(M, 1, 2), np.concatenate([cost, np.zeros((B, m))], axis=1), lo, hi, kind=kind)
    z = np.asarray(res["z"])
    return np.asarray(res["status"]).astype(np.int32), z[:, :d], z[:, d:]


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
    trips = [tuple(np.asarray(a, dtype=np.float64) for a in _trip(p)) for p in polys]
    trips = [(np.atleast_2d(A), l, u) for A, l, u in trips]
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
    if todo and route == "polyhedron" and callable(getattr(engine, "exemplar_polys", None)):
        todo = _exemplar_slack_polyhedra(todo, trips, opens, engine, tol, slack_cap, strict, empty, example, eps_out)
    if todo and _has_lps(engine):
        # closed polyhedra: the answer depends on eps alone -- the LP solver; with an open bound it depends on which duals the
        # solver returns: today's route
        closed = [b for b in todo if not opens[b][0].any() and not opens[b][1].any()]
        todo = [b for b in todo if opens[b][0].any() or opens[b][1].any()]
        _exemplar_slack_lps(closed, trips, engine, tol, slack_cap, strict, empty, example, eps_out)
    if todo:
        dmax = max(trips[b][0].shape[1] for b in todo) + 1
        mmax = max(2 * trips[b][0].shape[0] for b in todo) + 1
        A2 = np.zeros((len(todo), mmax, dmax)); l2 = np.full((len(todo), mmax), -INF); u2 = np.full((len(todo), mmax), INF)
        cost = np.zeros((len(todo), dmax)); cost[:, dmax - 1] = 1.0
        for k, b in enumerate(todo):
            A, l, u = trips[b]
            n, d = A.shape
            A2[k, :n, :d] = A; A2[k, :n, dmax - 1] = 1.0; l2[k, :n] = l                    # A x + eps >= l
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
    rest = []
    for b, p in enumerate(polys):
        if x is not None and hasattr(p, "contains") and p.contains(np.asarray(x, dtype=np.float64)):
            continue
        rest.append(b)
    if rest:
        e, _, _ = exemplar_slack_batch([polys[b] for b in rest], engine, tol=tol, route=route)
        out[rest] = e
    return out


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
    trips = [tuple(np.asarray(a, dtype=np.float64) for a in _trip(p)) for p in polys]
    trips = [(np.atleast_2d(A), l, u) for A, l, u in trips]
    if route == "polyhedron" and trips and callable(getattr(engine, "implicit_bounds", None)):
        return _implicit_bounds_polyhedra(trips, engine, tol)
    return _implicit_bounds_jobs(trips, engine, tol)


def _implicit_bounds_polyhedra(trips, engine, tol):
    """implicit_bounds_batch on an engine with `implicit_bounds`: the polyhedra packed by shape (rows, columns), one call per
    shape; an EMPTY polyhedron raises "Empty set" for the lowest-numbered one, any other status the error that names the
    polyhedron and the row whose solve ended it.  Shapes beyond the kernel's limits go the route of the jobs."""
    from .engine import colmajor
    packs, beyond = {}, []
    for b, (A, l, u) in enumerate(trips):
        r, d = A.shape
        if r < 1 or d < 1 or r > LP_MAX_R or d > LP_MAX_D:
            beyond.append(b)
        else:
            packs.setdefault((r, d), []).append(b)
    out = [None] * len(trips)
    empty, failed = [], []
    for (r, d), members in sorted(packs.items()):
        k = len(members)
        A = np.stack([trips[b][0] for b in members]).reshape(k, r, d)
        l = np.stack([trips[b][1] for b in members]).reshape(k, r); u = np.stack([trips[b][2] for b in members]).reshape(k, r)
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
    if jobs and _has_lps(engine):
        ext = _row_extremes_lps(trips, jobs, engine, nm)
        jobs = []
        _implicit_from_extremes(trips, out, ext, tol)
    if jobs:
        dmax = max(trips[b][0].shape[1] for b, _, _ in jobs); mmax = max(trips[b][0].shape[0] for b, _, _ in jobs)
        A2 = np.zeros((len(jobs), mmax, dmax)); l2 = np.full((len(jobs), mmax), -INF); u2 = np.full((len(jobs), mmax), INF)
        cost = np.zeros((len(jobs), dmax))
        big = np.zeros(len(jobs))
        for k, (b, i, sg) in enumerate(jobs):
            A, l, u = trips[b]
            n, d = A.shape
            A2[k, :n, :d] = A; l2[k, :n] = l; u2[k, :n] = u
            cost[k, :d] = sg * A[i]
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


def _has_lps(engine):
    return callable(getattr(engine, "solve_lps", None))


def _row_extremes_lps(trips, jobs, engine, nm=lambda b: b):
    """implicit_bounds_batch's LPs on an engine with `solve_lps`: the polyhedra that have jobs are packed by shape (rows,
    columns) and go up once per pack; a job names its objective by (row, sign), so no cost vector and no copy of the
    polyhedron is made for it; an unbounded row is the solver's own answer.  jobs: [(polyhedron, row, sign)].
    -> {(b, i, sign): the extreme of a_i'x, -+inf when unbounded}."""
    from .engine import colmajor
    packs = {}
    for b, i, sg in jobs:
        packs.setdefault(trips[b][0].shape, {}).setdefault(b, []).append((i, sg))
    ext = {}
    for (r, d), of in sorted(packs.items()):
        members = sorted(of)
        A = np.stack([trips[b][0] for b in members]).reshape(len(members), r, d)
        l = np.stack([trips[b][1] for b in members]).reshape(len(members), r); u = np.stack([trips[b][2] for b in members]).reshape(len(members), r)
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
    packs = {}
    for b in items:
        packs.setdefault(trips[b][0].shape, []).append(b)
    for (n, d), members in sorted(packs.items()):
        k = len(members)
        A = np.stack([trips[b][0] for b in members]).reshape(k, n, d)
        A2 = np.zeros((k, 2 * n + 1, d + 1)); l2 = np.empty((k, 2 * n + 1))
        A2[:, :n, :d] = A; A2[:, n:2 * n, :d] = -A; A2[:, :, d] = 1.0
        l2[:, :n] = np.stack([trips[b][1] for b in members]).reshape(k, n); l2[:, n:2 * n] = -np.stack([trips[b][2] for b in members]).reshape(k, n)
        l2[:, 2 * n] = -slack_cap
        res = engine.solve_lps(colmajor(A2), l2, np.full((k, 2 * n + 1), INF), np.arange(k, dtype=np.int32),
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
    packs, beyond = {}, []
    for b in items:
        n, d = trips[b][0].shape
        if n < 1 or d < 1 or n > EX_MAX_N or d > EX_MAX_D:
            beyond.append(b)
        else:
            packs.setdefault((n, d), []).append(b)
    failed = []
    for (n, d), members in sorted(packs.items()):
        k = len(members)
        A = np.stack([trips[b][0] for b in members]).reshape(k, n, d)
        l = np.stack([trips[b][1] for b in members]).reshape(k, n); u = np.stack([trips[b][2] for b in members]).reshape(k, n)
        ol = np.stack([opens[b][0] for b in members]).reshape(k, n).astype(np.uint8)
        oh = np.stack([opens[b][1] for b in members]).reshape(k, n).astype(np.uint8)
        res = engine.exemplar_polys(colmajor(A), l, u, ol, oh, tol=tol, slack_cap=slack_cap)
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


# ---- the LP solver (qpn_solve_lps): bounded-variable primal simplex, the numpy twin -----------------------------------------
LP_OPTIMAL, LP_INFEASIBLE, LP_UNBOUNDED, LP_ITER_LIMIT, LP_FAILURE = 1, 2, 3, 4, 5
LP_PIV_BAND = 1.0 - 2.0 ** -30                  # pivot / pricing candidates within this factor of the best count as equal
LP_RATIO_TIE = 1e-12                            # ratios within this (relative, at least absolute) of the smallest count as tied
LP_BLAND_AFTER = 20                             # consecutive zero-length steps before the lowest eligible id enters
LP_DEFAULT_OPTS = dict(piv_tol=1e-9, feas_tol=1e-9, opt_tol=1e-9, check_tol=1e-6, max_iters=0)
LP_MAX_D, LP_MAX_R = 256, 1024


def _lp_pivot(T, i, j):
    """Exchange the basic variable of row i and the nonbasic one of column j of the dictionary T [r + 1, d] (cost row last)."""
    p = T[i, j]
    col = T[:, j].copy()
    new = -T[i, :] / p
    new[j] = 1.0 / p
    T += col[:, None] * new[None, :]
    T[:, j] = col / p
    T[i, :] = new


class _LpState:
    """What a solve leaves for the next one over the same polyhedron: the dictionary T [r + 1, d] (cost row last), the ids of the
    basic (rb) and nonbasic (cn) variables, the nonbasic values xn; and what the last loop left for the check (xb, g, dj, e, dirn, a)."""


def _lp_setup(A, l, u, c, o):
    """Steps 0-4 of qpn_solve_lps: the data screen, scaling, the dictionary, the crash, the nonbasic values.  -> _LpState; S.nonfinite
    is set when step 0 fails the job; S.zbad is the all-zero row outside its bounds that settles the job (its unit Farkas vector in
    S.zlam), or None."""
    r, d = A.shape
    S = _LpState()
    S.A, S.l, S.u, S.r, S.d, S.o = A, l, u, r, d, o
    S.max_iters = o["max_iters"] if o["max_iters"] > 0 else 50 * (r + d) + 100
    S.zbad, S.iters, S.e, S.dirn, S.a, S.g, S.dj, S.xb = None, 0, -1, 0.0, None, None, None, np.zeros(r)
    piv_tol = o["piv_tol"]
    with np.errstate(all="ignore"):
        # 0. the data screen: an entry of A or c that is not finite, a bound that is not a number, l = +inf or u = -inf
        S.nonfinite = not bool(np.all(np.abs(A) < INF) and np.all(np.abs(c) < INF) and np.all(l < INF) and np.all(u > -INF))
        if S.nonfinite:
            return S
        # 1. row scaling; an all-zero row outside its bounds settles the job
        amax = np.max(np.abs(A), axis=1)
        S.amax = amax
        for i in range(r):
            if amax[i] == 0.0 and (u[i] < 0.0 or l[i] > 0.0):
                S.zbad = i
                S.zlam = np.zeros(r)
                S.zlam[i] = 1.0 if u[i] < 0.0 else -1.0
                return S
        sc = np.ones(r)
        nz = amax > 0.0
        sc[nz] = 1.0 / amax[nz]
        ls, us = l * sc, u * sc
        # 2. the dictionary: basic = T nonbasic, the cost row below it
        T = np.empty((r + 1, d))
        T[:r] = A * sc[:, None]
        T[r] = c
        rb = d + np.arange(r); cn = np.arange(d)
        # 3. crash: the x come into the basis, column by column
        for j in range(d):
            col = np.where(rb >= d, np.abs(T[:r, j]), 0.0)
            best = np.max(col)
            if not best > piv_tol:
                continue
            i = int(np.nonzero((rb >= d) & (col >= best * LP_PIV_BAND))[0][0])
            _lp_pivot(T, i, j)
            rb[i], cn[j] = cn[j], rb[i]
        # 4. nonbasic values
        xn = np.zeros(d)
        for j in range(d):
            if cn[j] >= d:
                lo, hi = ls[cn[j] - d], us[cn[j] - d]
                if np.isfinite(lo) and np.isfinite(hi):
                    xn[j] = lo if abs(lo) <= abs(hi) else hi
                elif np.isfinite(lo):
                    xn[j] = lo
                elif np.isfinite(hi):
                    xn[j] = hi
    S.sc, S.ls, S.us, S.T, S.rb, S.cn, S.xn = sc, ls, us, T, rb, cn, xn
    return S


def _lp_loop(S, iters0=0):
    """Steps 5-8: the simplex loop from the state's dictionary, with a fresh degeneracy counter and the step counter at iters0 (the
    steps of the loop before a rebuild count against the same max_iters).  -> status; the steps in S.iters, the basic values,
    violations and reduced costs of the last round in S.xb, S.g, S.dj, the last entering column and direction in S.e, S.dirn, S.a."""
    r, d, T, rb, cn, xn, ls, us = S.r, S.d, S.T, S.rb, S.cn, S.xn, S.ls, S.us
    piv_tol, feas_tol, opt_tol, max_iters = S.o["piv_tol"], S.o["feas_tol"], S.o["opt_tol"], S.max_iters
    with np.errstate(all="ignore"):
        status, iters, degen = LP_FAILURE, iters0, 0
        e, dirn, a, g, dj = -1, 0.0, None, None, None
        while True:
            lob = np.where(rb >= d, ls[np.maximum(rb - d, 0)], -INF); upb = np.where(rb >= d, us[np.maximum(rb - d, 0)], INF)
            lon = np.where(cn >= d, ls[np.maximum(cn - d, 0)], -INF); upn = np.where(cn >= d, us[np.maximum(cn - d, 0)], INF)
            xb = np.zeros(r)
            for j in range(d):                          # (a nonbasic at 0 adds nothing)
                if xn[j] != 0.0:
                    xb = xb + T[:r, j] * xn[j]
            below = xb < lob - feas_tol * np.maximum(1.0, np.abs(lob))
            above = xb > upb + feas_tol * np.maximum(1.0, np.abs(upb))
            g = np.where(below, -1.0, np.where(above, 1.0, 0.0))
            phase1 = bool(np.any(g != 0.0))
            if phase1:                                  # 5. the gradient of the sum of violations
                dj = np.zeros(d)
                for i in range(r):
                    if g[i] != 0.0:
                        dj = dj + g[i] * T[i, :]
            else:
                dj = T[r].copy()
            # 6. the entering variable
            free = lon != upn
            inc = (dj < -opt_tol) & (xn < upn) & free
            dec = (dj > opt_tol) & (xn > lon) & free
            elig = inc | dec
            if not elig.any():
                status = LP_INFEASIBLE if phase1 else LP_OPTIMAL
                break
            if degen >= LP_BLAND_AFTER:
                pick = elig
            else:
                mag = np.where(elig, np.abs(dj), 0.0)
                pick = elig & (mag >= np.max(mag) * LP_PIV_BAND)
            e = int(np.argmin(np.where(pick, cn, r + d)))
            dirn = 1.0 if inc[e] else -1.0
            # 7. the ratio test
            a = T[:r, e] * dirn
            tgt = np.where(a > 0.0, np.where(below, lob, np.where(above, INF, upb)), np.where(above, upb, np.where(below, -INF, lob)))
            ratio = np.where(np.abs(a) > piv_tol, np.maximum((tgt - xb) / a, 0.0), INF)
            tflip = upn[e] - xn[e] if dirn > 0.0 else xn[e] - lon[e]
            tmin = min(tflip, np.min(ratio)) if r else tflip
            if not tmin < INF:
                status = LP_FAILURE if phase1 else LP_UNBOUNDED
                break
            thr = tmin + LP_RATIO_TIE * max(1.0, tmin)
            win = int(np.min(np.where(ratio <= thr, rb, r + d))) if r else r + d
            if tflip <= thr and cn[e] < win:
                win = int(cn[e])
            if win == r + d:                            # (not-a-number data: no candidate compares)
                status = LP_FAILURE
                break
            if iters >= max_iters:                      # a step is due and none is left: a job that ends within max_iters keeps its outcome
                status = LP_ITER_LIMIT
                break
            iters += 1
            degen = degen + 1 if tmin == 0.0 else 0
            if win == cn[e]:
                xn[e] = upn[e] if dirn > 0.0 else lon[e]
            else:
                i = int(np.nonzero(rb == win)[0][0])
                _lp_pivot(T, i, e)                      # 8.
                rb[i], cn[e] = cn[e], rb[i]
                xn[e] = tgt[i]
    S.iters, S.e, S.dirn, S.a, S.g, S.dj, S.xb = iters, e, dirn, a, g, dj, xb
    return status


def _lp_point(S, c):
    """Step 9, first half: the point the loop ended at, on the unscaled data.  -> (x [d], obj = c'x)."""
    x = np.zeros(S.d)
    with np.errstate(all="ignore"):
        for j in range(S.d):
            if S.cn[j] < S.d:
                x[S.cn[j]] = S.xn[j]
        for i in range(S.r):
            if S.rb[i] < S.d:
                x[S.rb[i]] = S.xb[i]
        obj = 0.0
        for k in range(S.d):
            obj = obj + c[k] * x[k]
    return x, obj


def _lp_check(S, status, c, x):
    """Step 9, second half: the check of what an OPTIMAL / UNBOUNDED / INFEASIBLE end claims, on the unscaled data at check_tol.
    -> (ok, lambda [r], ray [d])."""
    A, l, u, r, d, rb, cn, sc, amax = S.A, S.l, S.u, S.r, S.d, S.rb, S.cn, S.sc, S.amax
    ct = S.o["check_tol"]
    e, dirn, a, g, dj = S.e, S.dirn, S.a, S.g, S.dj
    lam = np.zeros(r); ray = np.zeros(d)
    with np.errstate(all="ignore"):
        s = np.zeros(r)
        for j in range(d):
            s = s + A[:, j] * x[j]
        tl = ct * np.maximum(1.0, np.abs(l)); tu = ct * np.maximum(1.0, np.abs(u))
        ok = True
        if status != LP_INFEASIBLE:
            ok = bool(np.all((s >= l - tl) & (s <= u + tu)))
        if status == LP_OPTIMAL:
            for j in range(d):
                if cn[j] >= d:
                    lam[cn[j] - d] = dj[j] * sc[cn[j] - d]
            for k in range(d):
                acc = 0.0
                for i in range(r):
                    acc = acc + A[i, k] * lam[i]
                ok = ok and bool(abs(c[k] - acc) <= ct * max(1.0, abs(c[k])))
            ok = ok and bool(np.all(~(lam > ct) | (np.abs(s - l) <= tl)) and np.all(~(lam < -ct) | (np.abs(s - u) <= tu)))
        elif status == LP_UNBOUNDED:
            if cn[e] < d:
                ray[cn[e]] = dirn
            for i in range(r):
                if rb[i] < d:
                    ray[rb[i]] = a[i]
            cr = 0.0
            for k in range(d):
                cr = cr + c[k] * ray[k]
            ar = np.zeros(r)
            for j in range(d):
                ar = ar + A[:, j] * ray[j]
            tr = ct * max(1.0, float(np.max(np.abs(ray)))) * amax
            ok = ok and bool(cr < 0.0) and bool(np.all(~np.isfinite(l) | (ar >= -tr)) and np.all(~np.isfinite(u) | (ar <= tr)))
        else:
            for i in range(r):
                if rb[i] >= d:
                    lam[rb[i] - d] = g[i] * sc[rb[i] - d]
            for j in range(d):
                if cn[j] >= d:
                    k = cn[j] - d
                    y = -dj[j]
                    if (y > 0.0 and not np.isfinite(u[k])) or (y < 0.0 and not np.isfinite(l[k])):
                        y = 0.0
                    lam[k] = y * sc[k]
            ymax = max(1.0, float(np.max(np.abs(lam)))) if r else 1.0
            for k in range(d):
                acc = 0.0
                for i in range(r):
                    acc = acc + A[i, k] * lam[i]
                ok = ok and bool(abs(acc) <= ct * ymax)
            # the Farkas sum is negative by more than every bound relaxed by the tolerance primal feasibility is judged at accounts for
            bound, slack = 0.0, 0.0
            for i in range(r):
                if lam[i] > 0.0:
                    bound = bound + lam[i] * u[i]
                    slack = slack + lam[i] * tu[i]
                elif lam[i] < 0.0:
                    bound = bound + lam[i] * l[i]
                    slack = slack - lam[i] * tl[i]
            ok = ok and bool(bound < -slack)
    return ok, lam, ray


def _lp_rebuild(S, c):
    """The dictionary of the current basis once more from the scaled rows (step 10): T = A * sc with the cost row c, every x
    nonbasic; then, for the columns j ascending whose x is basic in the current basis (a row's id stands in column j), the crash's
    pivot restricted to the rows whose id is nonbasic in the current basis and still basic here: the largest |T[i, j]|, the lowest
    i within PIV_BAND of it.  At most d pivots.  The nonbasic rows keep their values.  -> False when a pivot is not above piv_tol."""
    r, d, T, rb, cn, xn = S.r, S.d, S.T, S.rb, S.cn, S.xn
    with np.errstate(all="ignore"):
        out = np.zeros(r, bool); val = np.zeros(r)
        for j in range(d):
            if cn[j] >= d:
                out[cn[j] - d] = True; val[cn[j] - d] = xn[j]
        want = cn >= d                                  # (a nonbasic x never left its own column)
        T[:r] = S.A * S.sc[:, None]
        T[r] = c
        rb[:] = d + np.arange(r); cn[:] = np.arange(d)
        for j in range(d):
            if not want[j]:
                continue
            cand = out & (rb >= d)
            col = np.where(cand, np.abs(T[:r, j]), 0.0)
            best = np.max(col)
            if not best > S.o["piv_tol"]:
                return False
            i = int(np.nonzero(cand & (col >= best * LP_PIV_BAND))[0][0])
            _lp_pivot(T, i, j)
            rb[i], cn[j] = cn[j], rb[i]
        for j in range(d):
            if cn[j] >= d:
                xn[j] = val[cn[j] - d]
    return True


def _lp_finish(S, c, cold):
    """Steps 5-10 from the state's dictionary: the loop, the point and step 9's check; an end that is not certified -- a FAILURE of
    the loop, an INFEASIBLE end of a warm solve (the polyhedron has a point), a certificate that fails -- rebuilds the dictionary
    (_lp_rebuild) and runs the loop once more, the step counter going on; what that ends with stands.  cold: an INFEASIBLE end is
    an outcome (checked like the others), and with cold == "feasible" an OPTIMAL end is taken unchecked (c = 0: lp_feasible).
    -> (status, x, obj, lambda, ray); every status but a certified one comes with lambda = ray = 0."""
    r, d = S.r, S.d
    iters0 = 0
    for attempt in (0, 1):
        status = _lp_loop(S, iters0)
        iters0 = S.iters
        x, obj = _lp_point(S, c)
        if status == LP_ITER_LIMIT:
            return status, x, obj, np.zeros(r), np.zeros(d)
        if status == LP_OPTIMAL and cold == "feasible":
            return status, x, obj, np.zeros(r), np.zeros(d)
        if status in (LP_OPTIMAL, LP_UNBOUNDED) or (status == LP_INFEASIBLE and cold):
            ok, lam, ray = _lp_check(S, status, c, x)
            if ok:
                return status, x, obj, lam, ray
        if attempt == 1 or not _lp_rebuild(S, c):
            break
    return LP_FAILURE, x, obj, np.zeros(r), np.zeros(d)


def _lp_one(A, l, u, c, o):
    """One LP  min c'x  s.t.  l <= A x <= u  (A [r, d] math layout) by the method of qpn_solve_lps (include/qpn_hip.h states it):
    set-up, then loop, check and at most one rebuild (_lp_finish) -- the parts issubset_pairs_host runs too.
    -> (status, x [d], obj, lambda [r], ray [d], iters)."""
    S = _lp_setup(A, l, u, c, o)
    if S.nonfinite:
        return LP_FAILURE, np.zeros(S.d), 0.0, np.zeros(S.r), np.zeros(S.d), 0
    if S.zbad is not None:
        return LP_INFEASIBLE, np.zeros(S.d), 0.0, S.zlam, np.zeros(S.d), 0
    status, x, obj, lam, ray = _lp_finish(S, c, True)
    return status, x, obj, lam, ray, S.iters


def _lp_feasible(A, l, u, o):
    """The feasibility solve of issubset_pairs_host (a) and implicit_bounds_host (a) (the kernel's lp_feasible): steps 0-8 and 10
    with c = 0.  Data the screen rejects is LP_FAILURE at 0 steps; an infeasible all-zero row, or an INFEASIBLE end whose Farkas
    certificate holds, is LP_INFEASIBLE; one whose certificate fails after the rebuild too LP_FAILURE.
    -> (LP_OPTIMAL / LP_INFEASIBLE / LP_ITER_LIMIT / LP_FAILURE, S, x [d]); the steps in S.iters."""
    zero = np.zeros(A.shape[1])
    S = _lp_setup(A, l, u, zero, o)
    if S.nonfinite:
        return LP_FAILURE, S, zero
    if S.zbad is not None:
        return LP_INFEASIBLE, S, zero
    status, x, _, _, _ = _lp_finish(S, zero, "feasible")
    return status, S, x


def _lp_resolve(S, c):
    """The solve of objective c from the basis the previous solve over the polyhedron left (the kernel's lp_resolve): the cost
    row of c in the current dictionary (issubset_pairs_host (e)), then _lp_finish: the loop with fresh step and degeneracy counters,
    the point, step 9's check and, where the end is not certified, the rebuild and the loop once more.  -> (LP_OPTIMAL or
    LP_UNBOUNDED, certified / LP_ITER_LIMIT / LP_FAILURE: a FAILURE of the loop, an INFEASIBLE end, a certificate that fails, after
    the rebuild too; x [d]; obj = c'x); the steps in S.iters."""
    T, rb, cn, r, d = S.T, S.rb, S.cn, S.r, S.d
    with np.errstate(all="ignore"):
        row = np.zeros(d)
        for i in range(r):
            if rb[i] < d:
                row = row + c[rb[i]] * T[i, :]
        for j in range(d):
            if cn[j] < d:
                row[j] = row[j] + c[cn[j]]
        T[r] = row
    status, x, obj, _, _ = _lp_finish(S, c, False)
    return status, x, obj


def solve_lps_host(Ac, l, u, poly_of, cost=None, obj_row=None, obj_sign=None, opts=None):
    """The numpy twin of Engine.solve_lps (qpn_solve_lps), the normative statement of the method: the kernel does the same
    operations in the same order (every sum over the ascending index as acc = acc + a * b, no contraction), so every output is
    bit-equal.  Ac [polys, d, r] (the polyhedra's matrices in the ABI layout), l, u [polys, r] (+-inf allowed), poly_of [jobs];
    the objective of job t is cost[t] or, without `cost`, obj_sign[t] * row obj_row[t] of its polyhedron.
    -> dict(status [jobs] int32, x [jobs, d], obj [jobs], lam [jobs, r], ray [jobs, d], iters [jobs] int32).  A job whose
    poly_of / obj_row is out of range answers LP_FAILURE with zeros (the kernel's rule for device index arrays), and so does one
    whose data the screen of step 0 rejects; every LP_FAILURE and LP_ITER_LIMIT has lam = ray = 0."""
    Ac = np.asarray(Ac, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    polys, d, r = Ac.shape
    poly_of = np.asarray(poly_of, dtype=np.int64)
    jobs = len(poly_of)
    o = dict(LP_DEFAULT_OPTS)
    o.update(opts or {})
    out = dict(status=np.zeros(jobs, np.int32), x=np.zeros((jobs, d)), obj=np.zeros(jobs), lam=np.zeros((jobs, r)),
               ray=np.zeros((jobs, d)), iters=np.zeros(jobs, np.int32))
    for t in range(jobs):
        b = int(poly_of[t])
        row_ok = cost is not None or 0 <= int(obj_row[t]) < r
        if not (0 <= b < polys) or not row_ok:
            out["status"][t] = LP_FAILURE
            continue
        A = np.ascontiguousarray(Ac[b].T)
        c = np.asarray(cost[t], dtype=np.float64) if cost is not None else float(obj_sign[t]) * A[int(obj_row[t])]
        st, x, obj, lam, ray, it = _lp_one(A, l[b], u[b], c, o)
        out["status"][t] = st; out["x"][t] = x; out["obj"][t] = obj; out["lam"][t] = lam; out["ray"][t] = ray; out["iters"][t] = it
    return out


# ---- subset tests (qpn_issubset_pairs): one job per pair, the numpy twin ---------------------------------------------------------
SUBSET_HOLDS, SUBSET_BY_POINT, SUBSET_BY_OPTIMUM, SUBSET_UNBOUNDED, SUBSET_ITER_LIMIT, SUBSET_FAILURE, SUBSET_EMPTY = 0, 1, 2, 3, 4, 5, 6


def _subset_one(A1, l1, u1, A2, l2, u2, tol, o):
    """One pair P1 ⊆ P2 by the method of qpn_issubset_pairs (A1 [r1, d], A2 [r2, d] math layout).
    -> (how, bound, val, lps, iters)."""
    d = A1.shape[1]
    # (a) the feasibility solve: steps 1-8 with c = 0
    status, S, x = _lp_feasible(A1, l1, u1, o)
    lps, iters = 1, S.iters
    if status != LP_OPTIMAL:
        return {LP_INFEASIBLE: SUBSET_EMPTY, LP_ITER_LIMIT: SUBSET_ITER_LIMIT}.get(status, SUBSET_FAILURE), -1, 0.0, lps, iters
    with np.errstate(all="ignore"):
        for i in range(A2.shape[0]):                        # (b) the bounds in order, the lower before the upper
            fl, fu = bool(np.abs(l2[i]) < INF), bool(np.abs(u2[i]) < INF)
            if not (fl or fu):
                continue
            # (c) rows of P1 equal to this one: the tightest of their bounds
            same = np.all(A1 == A2[i][None, :], axis=1)
            lo1, hi1 = -INF, INF
            for k in range(A1.shape[0]):
                if same[k]:
                    lo1 = max(lo1, l1[k]) if l1[k] == l1[k] else lo1
                    hi1 = min(hi1, u1[k]) if u1[k] == u1[k] else hi1
            for side in (0, 1):
                if side == 0:
                    if not fl or lo1 >= l2[i] - tol:
                        continue
                    c, beta = A2[i].copy(), l2[i]
                else:
                    if not fu or hi1 <= u2[i] + tol:
                        continue
                    c, beta = -A2[i], -u2[i]
                b = 2 * i + side
                # (d) the point the previous solve ended at
                v = 0.0
                for k in range(d):
                    v = v + c[k] * x[k]
                if v < beta - tol:
                    return SUBSET_BY_POINT, b, v, lps, iters
                # (e) the cost row of c in the current dictionary, (f) solve and decide
                lps += 1
                status, x, obj = _lp_resolve(S, c)
                iters += S.iters
                if status == LP_ITER_LIMIT:
                    return SUBSET_ITER_LIMIT, b, 0.0, lps, iters
                if status == LP_FAILURE:
                    return SUBSET_FAILURE, b, 0.0, lps, iters
                if status == LP_UNBOUNDED:
                    return SUBSET_UNBOUNDED, b, 0.0, lps, iters
                if obj < beta - tol:
                    return SUBSET_BY_OPTIMUM, b, obj, lps, iters
    return SUBSET_HOLDS, -1, 0.0, lps, iters                # (g)


def issubset_pairs_host(A1c, l1, u1, A2c, l2, u2, pi, pj, tol=1e-6, opts=None):
    """The numpy twin of Engine.issubset_pairs (qpn_issubset_pairs), the normative statement of the method; every output of the
    kernel is bit-equal to it.  Pair q asks whether first piece pi[q] ⊆ second piece pj[q].  A1c [B1, d, r1], A2c [B2, d, r2]
    (ABI layout), l1, u1 [B1, r1], l2, u2 [B2, r2] (+-inf allowed).

    (a) solve_lps_host's steps 1-8 on P1 with c = 0 (the crash and phase 1, once per pair; _lp_feasible); an INFEASIBLE end whose Farkas
    certificate holds is EMPTY (sub = 1, the convention of issubset_batch), otherwise FAILURE.  (b) the rows of P2 ascending, the
    lower bound (c = +a, beta = l2) before the upper (c = -a, beta = -u2), non-finite bounds skipped.  (c) a bound is skipped
    when rows of P1 equal the row of P2 entry by entry (==, unscaled) and the largest of their l1 is >= l2 - tol (the smallest of
    their u1 is <= u2 + tol).  (d) v = c'x at the point the previous solve ended at: v < beta - tol is BY_POINT.  (e) the cost
    row of c in the current dictionary: column j, acc = 0, over the rows i ascending with an x basic acc = acc + c[rb[i]] * T[i, j],
    then + c[cn[j]] when an x is nonbasic there.  (f) the loop with fresh step and degeneracy counters, step 9's check on P1
    ((e) and (f) are _lp_resolve):
    OPTIMAL with obj < beta - tol is BY_OPTIMUM, a certified ray UNBOUNDED, a failed certificate or an INFEASIBLE end that the
    rebuild and the second loop of _lp_finish do not mend FAILURE, ITER_LIMIT / FAILURE themselves.  (g) no bound left: HOLDS.
    -> dict(sub [pairs] uint8, how [pairs] int32 (SUBSET_*), bound [pairs] int32 (2 i + side of the deciding bound, -1 without),
    val [pairs] (the value that decided: BY_POINT, BY_OPTIMUM), lps [pairs] int32 (solves started, the feasibility solve counted),
    iters [pairs] int32 (all steps)).  A pair whose pi / pj is out of range answers FAILURE with bound -1 and zeros (the kernel's
    rule for device index arrays)."""
    A1c = np.asarray(A1c, dtype=np.float64); l1 = np.asarray(l1, dtype=np.float64); u1 = np.asarray(u1, dtype=np.float64)
    A2c = np.asarray(A2c, dtype=np.float64); l2 = np.asarray(l2, dtype=np.float64); u2 = np.asarray(u2, dtype=np.float64)
    B1, B2 = A1c.shape[0], A2c.shape[0]
    pi = np.asarray(pi, dtype=np.int64); pj = np.asarray(pj, dtype=np.int64)
    n = len(pi)
    o = dict(LP_DEFAULT_OPTS)
    o.update(opts or {})
    out = dict(sub=np.zeros(n, np.uint8), how=np.zeros(n, np.int32), bound=np.full(n, -1, np.int32), val=np.zeros(n),
               lps=np.zeros(n, np.int32), iters=np.zeros(n, np.int32))
    mats1, mats2 = {}, {}
    for q in range(n):
        a, b = int(pi[q]), int(pj[q])
        if not (0 <= a < B1 and 0 <= b < B2):
            out["how"][q] = SUBSET_FAILURE
            continue
        if a not in mats1:
            mats1[a] = np.ascontiguousarray(A1c[a].T)
        if b not in mats2:
            mats2[b] = np.ascontiguousarray(A2c[b].T)
        how, bound, val, lps, iters = _subset_one(mats1[a], l1[a], u1[a], mats2[b], l2[b], u2[b], float(tol), o)
        out["how"][q] = how; out["bound"][q] = bound; out["val"][q] = val; out["lps"][q] = lps; out["iters"][q] = iters
        out["sub"][q] = 1 if how in (SUBSET_HOLDS, SUBSET_EMPTY) else 0
    return out


# ---- implicit bounds (qpn_implicit_bounds): one job per polyhedron, the numpy twin ----------------------------------------------
IB_OK, IB_EMPTY, IB_ITER_LIMIT, IB_FAILURE = 0, 1, 2, 3
IB_HOW_UNDECIDED, IB_HOW_EXPLICIT, IB_HOW_IMPLICIT, IB_HOW_BY_POINTS, IB_HOW_BY_EXTREMES, IB_HOW_UNBOUNDED = 0, 1, 2, 3, 4, 5
IB_ALL_EXTREMES = 1


def _implicit_one(A, l, u, tol, flags, o):
    """One polyhedron by the method of qpn_implicit_bounds (A [r, d] math layout).
    -> (status, fail_row, eq [r] uint8, vals [r], how [r] int32, lo [r], hi [r], lps, iters)."""
    r, d = A.shape
    every = bool(flags & IB_ALL_EXTREMES)
    eq = np.zeros(r, np.uint8); vals = np.full(r, INF); how = np.full(r, IB_HOW_UNDECIDED, np.int32)
    lo = np.full(r, np.nan); hi = np.full(r, np.nan)
    with np.errstate(all="ignore"):
        # (0) explicit rows
        explicit = (np.abs(l - u) <= tol) | (l == u)
        eq[explicit] = 1; vals[explicit] = 0.5 * (l[explicit] + u[explicit]); how[explicit] = IB_HOW_EXPLICIT
        if np.any(~explicit & (l > u)):                     # crossed bounds: no LP is started
            return IB_EMPTY, -1, eq, vals, how, lo, hi, 0, 0
        # (a) the feasibility solve: steps 1-8 with c = 0
        status, S, x = _lp_feasible(A, l, u, o)
        lps, iters = 1, S.iters
        if status != LP_OPTIMAL:
            return {LP_INFEASIBLE: IB_EMPTY, LP_ITER_LIMIT: IB_ITER_LIMIT}.get(status, IB_FAILURE), -1, eq, vals, how, lo, hi, lps, iters

        def rows_at(x):                                     # A x on the unscaled rows, columns ascending
            s = np.zeros(r)
            for j in range(d):
                s = s + A[:, j] * x[j]
            return s

        # (b) the witnesses
        s = rows_at(x)
        wlo, whi = s.copy(), s.copy()
        # (c) the rows from the last
        for i in range(r - 1, -1, -1):
            if explicit[i]:
                continue
            if not every and whi[i] - wlo[i] > tol:
                how[i] = IB_HOW_BY_POINTS
                continue
            decided = False
            for side in (0, 1):
                c = A[i].copy() if side == 0 else -A[i]
                lps += 1
                status, x, obj = _lp_resolve(S, c)          # (the cost row of c in the current dictionary as in §5g (e))
                iters += S.iters
                if status == LP_ITER_LIMIT:
                    return IB_ITER_LIMIT, i, eq, vals, how, lo, hi, lps, iters
                if status == LP_FAILURE:
                    return IB_FAILURE, i, eq, vals, how, lo, hi, lps, iters
                s = rows_at(x)
                wlo = np.where(s < wlo, s, wlo); whi = np.where(s > whi, s, whi)
                if side == 0:
                    lo[i] = -INF if status == LP_UNBOUNDED else obj
                    if not every:
                        if status == LP_UNBOUNDED:
                            how[i] = IB_HOW_UNBOUNDED; decided = True
                            break
                        if whi[i] - lo[i] > tol:
                            how[i] = IB_HOW_BY_POINTS; decided = True
                            break
                else:
                    hi[i] = INF if status == LP_UNBOUNDED else -obj
            if decided:
                continue
            if abs(lo[i]) < INF and abs(hi[i]) < INF and abs(lo[i] - hi[i]) <= tol:
                eq[i] = 1; vals[i] = 0.5 * (hi[i] + lo[i]); how[i] = IB_HOW_IMPLICIT
            else:
                how[i] = IB_HOW_BY_EXTREMES if abs(lo[i]) < INF and abs(hi[i]) < INF else IB_HOW_UNBOUNDED
    return IB_OK, -1, eq, vals, how, lo, hi, lps, iters


def implicit_bounds_host(Ac, l, u, tol=1e-4, all_extremes=False, opts=None):
    """The numpy twin of Engine.implicit_bounds (qpn_implicit_bounds), the normative statement of the method; every output of
    the kernel is bit-equal to it.  `implicit_bounds` (src/sets.jl:660-713) with one job per polyhedron: Ac [polys, d, r] (ABI
    layout), l, u [polys, r] (+-inf allowed).

    (0) A row with |l - u| <= tol or l == u is EXPLICIT: eq = 1, val = 0.5 (l + u); no LP takes it as objective.  Another row
    with l > u makes the polyhedron EMPTY before any LP (lps = 0: the simplex keeps a nonbasic row at one of its bounds and would
    not see that they cross).  (a) solve_lps_host's steps 1-8 with c = 0 (the crash and phase 1, once; _lp_feasible): an infeasible all-zero row, or an INFEASIBLE end whose
    Farkas certificate holds, is EMPTY, a certificate that fails FAILURE, ITER_LIMIT itself; the polyhedron stops there, its other
    rows keep eq = 0, val = +inf, UNDECIDED.  (b) witnesses: s = A x at the end point on the unscaled rows, columns ascending
    (acc = acc + a * x); wlo = whi = s, and after every later solve whose certificate holds wlo = s where s < wlo, whi = s where
    s > whi.  (c) the rows r - 1 ... 0 that are not explicit: whi - wlo > tol is BY_POINTS without an LP; otherwise the minimum, c =
    +a_i from the current basis (the cost row as in issubset_pairs_host (e), fresh step and degeneracy counters, the loop, the
    point and step 9's check: _lp_resolve): a certified ray gives lo = -inf, UNBOUNDED; an optimum lo = obj, and whi - lo > tol is BY_POINTS;
    then the maximum with c = -a_i: hi = -obj or +inf.  eq = lo, hi finite and |lo - hi| <= tol: val = 0.5 (hi + lo), IMPLICIT;
    else BY_EXTREMES, or UNBOUNDED when one of the two is infinite.  ITER_LIMIT, or an INFEASIBLE end or a failed certificate that
    the rebuild and the second loop of _lp_finish do not mend, in one of these solves ends the polyhedron with that status and
    fail_row = i.  all_extremes (QPN_IB_ALL_EXTREMES): no BY_POINTS and
    no early exit after an unbounded minimum; every row that is not explicit gets both extremes and is decided by them alone.
    -> dict(status [polys] int32 (IB_*), fail_row [polys] int32 (-1 without), eq [polys, r] uint8, vals [polys, r] (+inf where eq
    = 0), how [polys, r] int32 (IB_HOW_*), lo, hi [polys, r] (NaN where no LP computed them), lps [polys] int32 (solves started,
    the feasibility solve counted), iters [polys] int32 (all steps))."""
    Ac = np.asarray(Ac, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    polys, d, r = Ac.shape
    o = dict(LP_DEFAULT_OPTS)
    o.update(opts or {})
    flags = IB_ALL_EXTREMES if all_extremes else 0
    out = dict(status=np.zeros(polys, np.int32), fail_row=np.full(polys, -1, np.int32), eq=np.zeros((polys, r), np.uint8),
               vals=np.full((polys, r), INF), how=np.zeros((polys, r), np.int32), lo=np.full((polys, r), np.nan),
               hi=np.full((polys, r), np.nan), lps=np.zeros(polys, np.int32), iters=np.zeros(polys, np.int32))
    for b in range(polys):
        got = _implicit_one(np.ascontiguousarray(Ac[b].T), l[b], u[b], float(tol), flags, o)
        for k, v in zip(("status", "fail_row", "eq", "vals", "how", "lo", "hi", "lps", "iters"), got):
            out[k][b] = v
    return out


# ---- emptiness with open bounds (qpn_exemplar_polys): one job per polyhedron, the numpy twin -------------------------------------
EX_MEMBER, EX_MEMBER_BAND, EX_EMPTY_SLACK, EX_EMPTY_OPEN, EX_ITER_LIMIT, EX_FAILURE = 0, 1, 2, 3, 4, 5
EX_MAX_N, EX_MAX_D = 511, 255


def exemplar_rows(A, l, u, slack_cap=1.0):
    """The slack LP of `exemplar` (src/sets.jl:608-619) over {x : l <= A x <= u} (A [n, d] math layout) in the variables (x, eps):
    rows i < n: [a_i, 1] >= l_i; rows n + i: [-a_i, 1] >= -u_i; row 2 n: eps >= -slack_cap.  -> (A2 [2 n + 1, d + 1], l2, u2 = +inf)."""
    n, d = A.shape
    A2 = np.zeros((2 * n + 1, d + 1)); l2 = np.empty(2 * n + 1)
    A2[:n, :d] = A; A2[n:2 * n, :d] = -A; A2[:, d] = 1.0
    l2[:n] = l; l2[n:2 * n] = -u; l2[2 * n] = -slack_cap
    return A2, l2, np.full(2 * n + 1, INF)


def _exemplar_one(A, l, u, open_lo, open_hi, tol, slack_cap, o):
    """One polyhedron by the method of qpn_exemplar_polys (A [n, d] math layout, open_lo / open_hi [n] bool).
    -> (empty, how, eps, x [d], row, lam [2 n + 1], iters)."""
    n, d = A.shape
    with np.errstate(all="ignore"):
        A2, l2, u2 = exemplar_rows(A, l, u, slack_cap)                      # (a)
        status, x, _, lam, _, iters = _lp_one(A2, l2, u2, 1.0 * A2[2 * n], o)
        if status != LP_OPTIMAL:                                            # (c)
            how = EX_ITER_LIMIT if status == LP_ITER_LIMIT else EX_FAILURE
            return 0, how, np.nan, np.zeros(d), -1, np.zeros(2 * n + 1), iters
        eps = x[d]                                                          # (b)
        row = -1
        if eps > tol:
            how = EX_EMPTY_SLACK
        elif eps > -tol:
            act_lo = (np.abs(lam[:n]) > tol) & open_lo & (np.abs(l) < INF)
            act_hi = (np.abs(lam[n:2 * n]) > tol) & open_hi & (np.abs(u) < INF)
            ids = np.concatenate([2 * np.nonzero(act_lo)[0], 2 * np.nonzero(act_hi)[0] + 1])
            how = EX_EMPTY_OPEN if ids.size else EX_MEMBER_BAND
            if ids.size:
                row = int(ids.min())
        else:
            how = EX_MEMBER
    empty = how in (EX_EMPTY_SLACK, EX_EMPTY_OPEN)
    return int(empty), how, eps, (np.zeros(d) if empty else x[:d]), row, lam, iters


def exemplar_polys_host(Ac, l, u, open_lo=None, open_hi=None, tol=1e-2, slack_cap=1.0, opts=None):
    """The numpy twin of Engine.exemplar_polys (qpn_exemplar_polys), the normative statement of the method; every output of the
    kernel is bit-equal to it.  `exemplar` / `isempty` (src/sets.jl:591-655) with one job per polyhedron: Ac [polys, d, n] (ABI
    layout), l, u [polys, n] (+-inf allowed), open_lo, open_hi [polys, n] (nonzero: that bound is open; None: closed).

    (a) The slack LP in (x, eps) (exemplar_rows): min eps over [a_i, 1] >= l_i, [-a_i, 1] >= -u_i, eps >= -slack_cap, the objective
    being the last row; solved as solve_lps_host solves a job (_lp_one: the data screen, the crash, the loop, step 9's check and
    at most one rebuild).  (b) On the certified optimum, eps = x[d]: eps > tol is EX_EMPTY_SLACK; eps > -tol is the band, where a
    bound is active when it is open, finite (an open flag on an infinite bound is ignored, src/sets.jl:354-356) and |lam_i| > tol
    (the lower bound of row i) or |lam_{n+i}| > tol (the upper): any active bound is EX_EMPTY_OPEN with row = the lowest 2 i +
    side, none EX_MEMBER_BAND; eps <= -tol is EX_MEMBER.  (c) LP_ITER_LIMIT is EX_ITER_LIMIT, every other end that is no certified
    optimum EX_FAILURE (the data screen included; the slack LP is feasible and bounded below, so INFEASIBLE and UNBOUNDED cannot be
    true answers): empty = 0, eps = NaN, x = 0, row = -1, lam = 0; iters is the count of the steps taken.
    -> dict(empty [polys] uint8, how [polys] int32 (EX_*), eps [polys], x [polys, d] (a member; zeros when empty or unanswered),
    row [polys] int32, lam [polys, 2 n + 1], iters [polys] int32)."""
    Ac = np.asarray(Ac, dtype=np.float64); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    polys, d, n = Ac.shape
    flags = [np.zeros((polys, n), bool) if f is None else np.asarray(f).reshape(polys, n) != 0 for f in (open_lo, open_hi)]
    o = dict(LP_DEFAULT_OPTS)
    o.update(opts or {})
    out = dict(empty=np.zeros(polys, np.uint8), how=np.zeros(polys, np.int32), eps=np.zeros(polys), x=np.zeros((polys, d)),
               row=np.full(polys, -1, np.int32), lam=np.zeros((polys, 2 * n + 1)), iters=np.zeros(polys, np.int32))
    for b in range(polys):
        got = _exemplar_one(np.ascontiguousarray(Ac[b].T), l[b], u[b], flags[0][b], flags[1][b], float(tol), float(slack_cap), o)
        for k, v in zip(("empty", "how", "eps", "x", "row", "lam", "iters"), got):
            out[k][b] = v
    return out
