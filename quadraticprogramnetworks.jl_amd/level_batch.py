"""A whole LEVEL of a QPNet as batches: the per-node map of process_qp (src/algorithm.jl:44-52), the sub-piece combinations
of src/qp_processing.jl:162-205 and the level's AVI step (solve_qep, src/avi.jl:382-444) served by O(1) device calls per
level and outer iteration, whatever the number of nodes.

The reference maps process_qp over the nodes of a level one by one and then forms ONE AVI for all of them
(src/avi.jl:399-400).  That AVI is block diagonal whenever the level's coupling graph is disconnected -- 5 000 followers
that read only their own leader are 5 000 independent node-AVIs, not one AVI of 320 000 unknowns -- so here

  * `components` splits the level's pool by the coupling graph (shared decision variables, or a player's KKT rows reading
    another player's decision variables: src/avi.jl:335-340 puts exactly those columns into M instead of N);
  * single-node components of equal shape are ONE batch of node records (qpn_solve_nodes / a resident qpn_nodes handle for
    nodes without children, whose records never change between outer iterations);
  * multi-node components of equal pool shape are ONE batch of pool AVIs (qpn_assemble_pools + qpn_solve_avi_batch);
  * `process_level` verifies every node of the level under every combination of its children's pieces in one
    qpn_verify_nodes call per record shape, and makes the solution-graph pieces of all optimal nodes with one
    comp_indices / recipes / pieces call each (src/avi.jl:447-477, src/avi_solutions.jl:200-215, :400-496).

A node's parameters are LOCAL here: only the variables its rows actually read (R, B have one column per such variable),
gathered from the iterate per sweep -- the reference's N = M[:, param_inds] over all n_total - n other variables
(src/avi.jl:340) is structurally zero outside them.

Everything numeric goes through the engine (the HIP library; the tests' CPU twin serves the same interface).
"""
from __future__ import annotations

import itertools
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np

from .programs import Poly, _positions

INF = np.inf
# A local piece enters a node's solution graph only when it contains the current point -- within MEMBER_TOL, tighter than
# verify_solution's accept band (1e-4, src/qp_processing.jl:57, :119) and far tighter than its feasibility tolerance (1e-3, :86).  comp_indices classifies with 1e-2 (src/avi_solutions.jl:511), so a row up to 1e-2 away
# from its bound still spawns the recipe "at the bound"; the reference keeps every such piece that is non-empty
# (src/avi_solutions.jl:247-249).  A piece the point misses by more than 1e-3 fails the PARENT's verify by construction (:86-89:
# infeasible), the parent's solve_qep then moves onto it, the next sweep finds the mirror image, and the loop ends in the
# reference's own "Cycling detected" (observed: one pair in 60 at n = m = 16).  Such pieces say nothing about optimality AT the
# point, so they are left out.  The tolerance has to sit BELOW the accept band: two neighbouring pieces' exact minimisers can lie
# 1e-4 apart (the parent optimal under B a hair inside B, and within 1e-3 of A's boundary): with a membership test as loose as
# verify's feasibility test each of the two points counts as a member of the other piece without being optimal there, and the
# parent is sent back and forth by 1e-4 for ever (observed: one pair in ~1 000 at n = m = 16).
MEMBER_TOL = 1e-5
CODE_TOL = 1e-4          # _refine_row_codes: a row keeps a code whose own condition the point meets within verify's tolerance (:57)
ROW_PAD = 16            # constraint rows of a record batch are padded with inert rows to a multiple of this (one MFMA tile)


# ---------------------------------------------------------------------------------------------------------------------
# node records
# ---------------------------------------------------------------------------------------------------------------------
def _static(qpn, pid: int) -> dict:
    """What a node's records owe to the net alone: decision indices, Q blocks, the base constraint rows."""
    cache = qpn.__dict__.setdefault("_node_static", {})
    st = cache.get(pid)
    if st is not None:
        return st
    qp = qpn.qps[pid]
    dec = np.asarray(qpn.decision_inds(pid), dtype=np.int64)
    base = [qpn.constraints[c].poly for c in qp.constraint_indices]
    f = qp.f
    supp = [f.row_support(dec)] + [P.support() for P in base]
    supp = np.unique(np.concatenate(supp)) if supp else np.zeros(0, np.int64)
    par = np.setdiff1d(supp, dec, assume_unique=True)
    st = dict(dec=dec, base=base, par=par, Qd=f.block(dec, dec), qd=f.q_at(dec),
              Ad=(np.vstack([P.block(dec) for P in base]) if base else np.zeros((0, dec.size))),
              l=(np.concatenate([P.l for P in base]) if base else np.zeros(0)),
              u=(np.concatenate([P.u for P in base]) if base else np.zeros(0)),
              # the blocks on the static parameters: what a record under child pieces that bring no new column keeps as it is
              R=f.block(dec, par), B=(np.vstack([P.block(par) for P in base]) if base else np.zeros((0, par.size))),
              reads=np.union1d(dec, par))
    cache[pid] = st
    return st


def _subtree_cols(qpn, pid: int) -> np.ndarray:
    """Every variable process_qp(pid) can read: the decision variables and static parameters of the node and of all nodes
    below it (the children's pieces are functions of exactly those)."""
    cache = qpn.__dict__.setdefault("_subtree_cols", {})
    got = cache.get(pid)
    if got is None:
        st = _static(qpn, pid)
        parts = [st["dec"], st["par"]] + [_subtree_cols(qpn, j) for j in sorted(qpn.network_edges[pid])]
        got = cache[pid] = np.unique(np.concatenate(parts))
    return got


def node_record(qpn, pid: int, child_polys: Sequence[Poly] = ()) -> dict:
    """Dense record of one node under one choice of its children's pieces (src/qp_processing.jl:62-66: the constraint
    stack is [base; child pieces]) with LOCAL parameters: dict(pid, dec, par, Qd, R, qd, Ad, B, l, u) in math layout."""
    st = _static(qpn, pid)
    dec = st["dec"]
    f = qpn.qps[pid].f
    if not child_polys:
        return dict(pid=pid, dec=dec, par=st["par"], Qd=st["Qd"], R=st["R"], qd=st["qd"], Ad=st["Ad"], B=st["B"], l=st["l"], u=st["u"])
    supp = [P.support() for P in child_polys]
    if all(_positions(st["reads"], c)[1].all() for c in supp):
        # the usual case: the children's pieces live on variables the node reads anyway (its own and its static parameters)
        par = st["par"]
        return dict(pid=pid, dec=dec, par=par, Qd=st["Qd"], R=st["R"], qd=st["qd"],
                    Ad=np.vstack([st["Ad"]] + [P.block(dec) for P in child_polys]),
                    B=np.vstack([st["B"]] + [P.block(par) for P in child_polys]),
                    l=np.concatenate([st["l"]] + [P.l for P in child_polys]),
                    u=np.concatenate([st["u"]] + [P.u for P in child_polys]))
    if child_polys:
        extra = np.unique(np.concatenate(supp))
        par = np.union1d(st["par"], np.setdiff1d(extra, dec, assume_unique=True))
        Ad = np.vstack([st["Ad"]] + [P.block(dec) for P in child_polys])
        l = np.concatenate([st["l"]] + [P.l for P in child_polys])
        u = np.concatenate([st["u"]] + [P.u for P in child_polys])
        cons = list(st["base"]) + list(child_polys)
    else:
        par, Ad, l, u, cons = st["par"], st["Ad"], st["l"], st["u"], st["base"]
    R = f.block(dec, par)
    B = np.vstack([P.block(par) for P in cons]) if cons else np.zeros((0, par.size))
    return dict(pid=pid, dec=dec, par=par, Qd=st["Qd"], R=R, qd=st["qd"], Ad=Ad, B=B, l=l, u=u)


def free_equalities(rec: dict) -> dict:
    """The same node with its equality rows (l = u) moved into the free block: an equality row's multiplier mu is a FREE variable
    of the node's AVI (src/avi.jl:113-128: the row a'x + b'w = e pairs with an unbounded multiplier), so z = [x; mu_E; lambda_I]
    with the free block [[Qd, -A_E'], [A_E, 0]] (right-hand side [qd; -e], parameter rows [R; B_E]) and the remaining rows
    [A_I 0] is the identical complementarity system.  The fused node kernels eliminate the free block without pivoting -- in this
    order: x first (Qd, definite), then mu (its block has become A_E Qd^-1 A_E', definite for independent rows) -- and run the
    complementary pivoting on the inequality rows alone; a record that keeps an equality row is declined by every one of them
    (the multiplier would have to be crashed in) and falls to the general kernel.  Every parent of a net has such rows: the
    stationarity rows of its children's pieces.  `nx` = the number of leading free variables that are decision variables."""
    l, u = rec["l"], rec["u"]
    eq = np.isfinite(l) & (l == u)
    if not eq.any():
        return rec
    E = np.nonzero(eq)[0]; I = np.nonzero(~eq)[0]
    n, ne = rec["Qd"].shape[0], E.size
    AE, BE = rec["Ad"][E], rec["B"][E]
    out = dict(rec)
    out["Qd"] = np.block([[rec["Qd"], -AE.T], [AE, np.zeros((ne, ne))]])
    out["R"] = np.vstack([rec["R"], BE])
    out["qd"] = np.concatenate([rec["qd"], -l[E]])
    out["Ad"] = np.hstack([rec["Ad"][I], np.zeros((I.size, ne))])
    out["B"] = rec["B"][I]
    out["l"], out["u"] = l[I], u[I]
    out["nx"] = n
    return out


class RecordBatch:
    """Records of equal shape (n, padded m, padded p) stacked in the ABI layout (column-major per item).  n counts the free
    block (Qd is n x n); its first nx entries are the node's decision variables (nx < n after free_equalities)."""

    def __init__(self, recs: List[dict], where: List[int], n: int, m: int, p: int):
        nb = len(recs)
        self.where = list(where)                     # positions of these records in the caller's list
        self.n, self.m, self.p = n, m, p
        self.m_true = np.array([len(r["l"]) for r in recs], dtype=np.int64)
        self.Qc = np.zeros((nb, n, n)); self.Rc = np.zeros((nb, p, n)); self.qd = np.zeros((nb, n))
        self.Ac = np.zeros((nb, n, m)); self.Bc = np.zeros((nb, p, m))
        self.l = np.full((nb, m), -INF); self.u = np.full((nb, m), INF)      # missing rows: 0'x in (-inf, inf) -- inert
        self.nx = recs[0]["dec"].size
        self.dec = np.zeros((nb, self.nx), dtype=np.int64)
        self.par = np.full((nb, p), -1, dtype=np.int64)                      # missing parameters: a zero column, w = 0
        mis = {len(r["l"]) for r in recs}; pis = {r["par"].size for r in recs}
        if len(mis) == 1 and len(pis) == 1:
            # the usual batch -- one row count, one parameter count: stacked and transposed in one go each
            mi, pi = mis.pop(), pis.pop()
            self.Qc[:] = np.stack([r["Qd"] for r in recs]).transpose(0, 2, 1)
            self.qd[:] = np.stack([r["qd"] for r in recs])
            self.dec[:] = np.stack([r["dec"] for r in recs])
            if pi:
                self.Rc[:, :pi] = np.stack([r["R"] for r in recs]).transpose(0, 2, 1)
                self.par[:, :pi] = np.stack([r["par"] for r in recs])
            if mi:
                self.Ac[:, :, :mi] = np.stack([r["Ad"] for r in recs]).transpose(0, 2, 1)
                self.l[:, :mi] = np.stack([r["l"] for r in recs]); self.u[:, :mi] = np.stack([r["u"] for r in recs])
                if pi:
                    self.Bc[:, :pi, :mi] = np.stack([r["B"] for r in recs]).transpose(0, 2, 1)
            recs = []
        for b, r in enumerate(recs):
            mi, pi = len(r["l"]), r["par"].size
            self.Qc[b] = r["Qd"].T
            self.Rc[b, :pi] = r["R"].T
            self.qd[b] = r["qd"]
            self.Ac[b, :, :mi] = r["Ad"].T
            self.Bc[b, :pi, :mi] = r["B"].T
            self.l[b, :mi] = r["l"]; self.u[b, :mi] = r["u"]
            self.dec[b] = r["dec"]; self.par[b, :pi] = r["par"]
        self.handle = None                           # resident copy (engine.upload_nodes), when the records are static
        self.handle_engine = None

    def __len__(self):
        return len(self.where)

    def gather(self, x):
        x = np.asarray(x, dtype=np.float64)
        xd = x[self.dec]
        w = np.where(self.par >= 0, x[np.maximum(self.par, 0)], 0.0)
        return xd, w

    def resident(self, engine, warm_mid=False):
        """The records as a resident handle of `engine` (made once), or None when the engine has no such thing.  warm_mid: a
        handle made by this call opts in to the warm start of the mid-size classes (Nodes.set_warm)."""
        if not hasattr(engine, "upload_nodes"):
            return None
        if self.handle is None or self.handle_engine is not engine:
            self.handle = engine.upload_nodes(self.Qc, self.Rc, self.qd, self.Ac, self.Bc, self.l, self.u)
            self.handle_engine = engine
            if warm_mid:
                self.handle.set_warm(1)
        return self.handle


def batch_records(recs: List[dict], row_pad: int = ROW_PAD) -> List[RecordBatch]:
    """Group records by (n, m rounded up to a multiple of row_pad); p is padded to the group's widest record (>= 1)."""
    groups: Dict[tuple, List[int]] = {}
    for i, r in enumerate(recs):
        m = len(r["l"])
        mp = max(row_pad, -(-m // row_pad) * row_pad) if m else 0
        groups.setdefault((r["Qd"].shape[0], mp, r["dec"].size), []).append(i)
    out = []
    for (n, mp, _nx), idx in sorted(groups.items()):
        p = max(1, max(recs[i]["par"].size for i in idx))
        out.append(RecordBatch([recs[i] for i in idx], idx, n, mp, p))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inner-node records from a static store, a pool of child pieces and column maps (qpn_assemble_parent_nodes)
# ---------------------------------------------------------------------------------------------------------------------
# "host": node_record -> (free_equalities) -> batch_records, per item in numpy, the records uploaded whole with every call.
# "device": on an engine with assemble_parent_nodes, solve_level (inner single-node components) and verify_items (items with
# children) send a static store once per net, the distinct child pieces and column maps once per call, and index arrays per
# item; the records are made in device memory and stay there for solve_nodes / verify_nodes.
PARENT_RECORDS_ROUTE = "host"
PARENT_SLOTS = 8               # child pieces per item (QPN_PARENT_SLOTS)
PARENT_MAX_ROWS = 1024         # rows of an item's constraint stack
# err words of assemble_parent_nodes; the lowest that applies
PR_OK, PR_BAD_INDEX, PR_BAD_MAP, PR_BAD_COLUMN, PR_BAD_ROWS, PR_BAD_EQ = 0, 1, 2, 3, 4, 5


def assemble_parent_records_host(form, ne, m, p, sQc, sRc, sqd, sAc, sBc, sl, su, mb_true, piece_desc, pA, pl, pu, map_off, map_data,
                                 parent_of, piece_of, map_of):
    """The numpy twin of Engine.assemble_parent_nodes (qpn_assemble_parent_nodes) and its normative statement: the records of
    many ITEMS, an item being one parent under one choice of its children's pieces (the constraint stack is [base; child
    pieces], src/qp_processing.jl:62-66), in the layout of RecordBatch.

      static store   per parent of one shape, ABI layout: sQc [P, n0, n0], sRc [P, ps, n0], sqd [P, n0], sAc [P, n0, mb],
                     sBc [P, ps, mb], sl, su [P, mb]; mb_true [P]: the parent's own base row count (mb is the common padded one)
      piece pool     piece_desc [pieces, 4] = (row0, rows, c, off): piece rows pl, pu [row0 : row0 + rows], coefficients
                     pA [off : off + rows * c] row-major over the piece's own c columns (Poly.local())
      column maps    map k = map_data [map_off[k] : map_off[k + 1]], one entry per piece column: j < n0 the decision column (Ad),
                     n0 + k (k < p) the parameter column (B), -1 a variable the parent does not read
      items          parent_of [items], piece_of / map_of [items, PARENT_SLOTS] (piece_of -1: empty slot)

    form 0 is node_record as RecordBatch stacks it (base rows, the slots' rows in slot order, inert rows up to m; parameter
    columns from ps on are zero); form 1 is free_equalities of it, E = the stack rows with finite l == u, which must number ne
    for every item.  Returns (Qc [items, n, n], Rc [items, p, n], qd [items, n], Ac [items, n, m], Bc [items, p, m], l, u
    [items, m], err [items] int32 (PR_*)), n = n0 + ne.  A bad item's record is its parent's Qd, R, qd over inert rows (zeros
    when the parent index is bad)."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    i64 = lambda a: np.asarray(a, dtype=np.int64)
    sQc, sRc, sqd, sAc, sBc, sl, su, pA, pl, pu = (f64(a) for a in (sQc, sRc, sqd, sAc, sBc, sl, su, pA, pl, pu))
    mb_true, piece_desc, map_off, map_data, parent_of, piece_of, map_of = (i64(a) for a in (mb_true, piece_desc, map_off, map_data, parent_of,
                                                                                          piece_of, map_of))
    form, m, p = int(form), int(m), int(p)
    ne = int(ne) if form else 0
    P, n0 = sqd.shape
    ps, mb = sRc.shape[1], sl.shape[1]
    items, pieces, maps = parent_of.shape[0], piece_desc.shape[0], map_off.shape[0] - 1
    n, pk = n0 + ne, min(p, ps)
    Qc = np.zeros((items, n, n)); Rc = np.zeros((items, p, n)); qd = np.zeros((items, n))
    Ac = np.zeros((items, n, m)); Bc = np.zeros((items, p, m))
    l = np.full((items, m), -INF); u = np.full((items, m), INF)
    err = np.zeros(items, np.int32)
    # a map is judged once: its range inside map_data, every entry in [-1, n0 + p), no column named twice
    map_bad = np.zeros(max(maps, 0), bool)
    for k in range(maps):
        a, b = int(map_off[k]), int(map_off[k + 1])
        if a < 0 or b < a or b > map_data.size:
            map_bad[k] = True
            continue
        mv = map_data[a:b]
        named = mv[mv >= 0]
        map_bad[k] = bool(np.any((mv < -1) | (mv >= n0 + p))) or np.unique(named).size != named.size
    for b in range(items):
        pa = int(parent_of[b])
        pa_ok = 0 <= pa < P
        any1, any2, mbt = not pa_ok, False, 0
        if pa_ok:
            mbt = int(mb_true[pa])
            if mbt < 0 or mbt > mb:
                any1, mbt = True, 0
        over = mbt > PARENT_MAX_ROWS
        if over:
            mbt = 0
        T, slots = mbt, []
        for k in range(PARENT_SLOTS):
            q, rows = int(piece_of[b, k]), 0
            if q != -1:
                mp = int(map_of[b, k])
                if not (0 <= q < pieces and 0 <= mp < maps):
                    any1 = True
                else:
                    row0, r, c, off = (int(v) for v in piece_desc[q])
                    if min(row0, r, c, off) < 0 or row0 + r > pl.size or off + r * c > pA.size:
                        any1 = True
                    elif map_bad[mp] or int(map_off[mp + 1]) - int(map_off[mp]) != c:
                        any2 = True
                    else:
                        rows = r
                        slots.append((row0, r, c, off, int(map_off[mp])))
            over = over or rows > PARENT_MAX_ROWS - T
            if not over:
                T += rows
        e = PR_BAD_INDEX if any1 else PR_BAD_MAP if any2 else PR_BAD_ROWS if over else PR_OK
        if pa_ok:
            Qc[b, :n0, :n0] = sQc[pa]; Rc[b, :pk, :n0] = sRc[pa, :pk]; qd[b, :n0] = sqd[pa]
        if e == PR_OK:
            # the stack in math layout: rows over the parent's decision and parameter columns
            Ad = np.zeros((T, n0)); Bs = np.zeros((T, p)); ls = np.zeros(T); us = np.zeros(T)
            Ad[:mbt] = sAc[pa][:, :mbt].T; Bs[:mbt, :pk] = sBc[pa][:pk, :mbt].T
            ls[:mbt] = sl[pa, :mbt]; us[:mbt] = su[pa, :mbt]
            t = mbt
            for row0, r, c, off, mo in slots:
                A = pA[off:off + r * c].reshape(r, c)
                mv = map_data[mo:mo + c]
                if np.any(A[:, mv == -1] != 0):
                    e = PR_BAD_COLUMN
                    break
                dcol = (mv >= 0) & (mv < n0); pcol = mv >= n0
                Ad[t:t + r, mv[dcol]] = A[:, dcol]
                Bs[t:t + r, mv[pcol] - n0] = A[:, pcol]
                ls[t:t + r] = pl[row0:row0 + r]; us[t:t + r] = pu[row0:row0 + r]
                t += r
        if e == PR_OK:
            eq = np.isfinite(ls) & (ls == us) if form else np.zeros(T, bool)
            E = np.nonzero(eq)[0]; I = np.nonzero(~eq)[0]
            if I.size > m:
                e = PR_BAD_ROWS
            elif form and E.size != ne:
                e = PR_BAD_EQ
        if e == PR_OK:
            Qc[b, :n0, n0:] = Ad[E].T; Qc[b, n0:, :n0] = -Ad[E]              # Qd' = [[Qd, -A_E'], [A_E, 0]], column-major
            Rc[b, :, n0:] = Bs[E].T; qd[b, n0:] = -ls[E]
            Ac[b, :n0, :I.size] = Ad[I].T; Bc[b, :, :I.size] = Bs[I].T
            l[b, :I.size] = ls[I]; u[b, :I.size] = us[I]
        err[b] = e
    return Qc, Rc, qd, Ac, Bc, l, u, err


def _parent_route(eng) -> bool:
    return PARENT_RECORDS_ROUTE == "device" and callable(getattr(eng, "assemble_parent_nodes", None))


def _movers(eng):
    """(up, down): numpy array -> the engine's device and back; the identity for an engine that computes on the host."""
    if getattr(eng, "device", -1) >= 0:
        import torch
        return (lambda a: torch.as_tensor(np.ascontiguousarray(a), device=f"cuda:{eng.device}")), (lambda a: a.cpu().numpy())
    return (lambda a: a), np.asarray


class DeviceRecordBatch(RecordBatch):
    """A RecordBatch whose record arrays were made by assemble_parent_nodes and live where the engine computes (`dev`: Qc, Rc,
    qd, Ac, Bc, l, u).  The host metadata (where, m_true, dec, par, nx) is as RecordBatch has it; the record arrays come to the
    host only when something reads them (solution_pieces): one download fills them, bit-equal to the host route's."""

    def __init__(self, where, n, m, p, nx, m_true, dec, par, dev, movers):
        self.where = list(where)
        self.n, self.m, self.p, self.nx = n, m, p, nx
        self.m_true, self.dec, self.par = m_true, dec, par
        self.dev, (self.up, self.down) = tuple(dev), movers
        self._host = None
        self.handle = self.handle_engine = None

    def _arrays(self):
        if self._host is None:
            self._host = tuple(np.asarray(self.down(a)) for a in self.dev)
        return self._host

    Qc = property(lambda self: self._arrays()[0]); Rc = property(lambda self: self._arrays()[1])
    qd = property(lambda self: self._arrays()[2]); Ac = property(lambda self: self._arrays()[3])
    Bc = property(lambda self: self._arrays()[4]); l = property(lambda self: self._arrays()[5])
    u = property(lambda self: self._arrays()[6])

    def resident(self, engine, warm_mid=False):
        return None

    def solve(self, eng, w, z0):
        res = eng.solve_nodes(*self.dev, self.up(w), z0=self.up(z0))
        return dict(status=self.down(res["status"]), z=self.down(res["z"]))

    def verify(self, eng, xd, w, tol):
        return tuple(self.down(a) for a in eng.verify_nodes(*self.dev, self.up(xd), self.up(w), tol=tol))


def _is_eq(l, u):
    return np.isfinite(l) & (l == u)


def _parent_store(qpn, n0: int, eng) -> dict:
    """The static store of every node of the net that has children and n0 decision variables: _static's blocks in the ABI
    layout, rows padded to the widest base, parameters to the widest list (>= 1).  Built once per net and shape, uploaded once
    per engine."""
    cache = qpn.__dict__.setdefault("_parent_store", {})
    S = cache.get(n0)
    if S is None:
        pids = [i for i in sorted(qpn.qps) if qpn.network_edges[i] and _static(qpn, i)["dec"].size == n0]
        sts = [_static(qpn, i) for i in pids]
        P = len(pids)
        mb = max([len(s["l"]) for s in sts], default=0); ps = max([1] + [s["par"].size for s in sts])
        Qc = np.zeros((P, n0, n0)); Rc = np.zeros((P, ps, n0)); qd = np.zeros((P, n0))
        Ac = np.zeros((P, n0, mb)); Bc = np.zeros((P, ps, mb)); l = np.full((P, mb), -INF); u = np.full((P, mb), INF)
        for k, s in enumerate(sts):
            mi, pi = len(s["l"]), s["par"].size
            Qc[k] = s["Qd"].T; Rc[k, :pi] = s["R"].T; qd[k] = s["qd"]
            Ac[k, :, :mi] = s["Ad"].T; Bc[k, :pi, :mi] = s["B"].T; l[k, :mi] = s["l"]; u[k, :mi] = s["u"]
        S = cache[n0] = dict(index={pid: k for k, pid in enumerate(pids)}, ps=ps, mb=mb,
                             arrays=(Qc, Rc, qd, Ac, Bc, l, u, np.array([len(s["l"]) for s in sts], np.int32)),
                             base_eq={pid: int(np.count_nonzero(_is_eq(s["l"], s["u"]))) for pid, s in zip(pids, sts)}, on=None)
    if S["on"] is None or S["on"][0] is not eng:
        up, _ = _movers(eng)
        S["on"] = (eng, tuple(up(a) for a in S["arrays"]))
    return S


def _parent_map(qpn, pid: int, st: dict, cols: np.ndarray):
    """Where the piece columns `cols` (sorted variable indices) land in parent pid's record: the map, int32.  Cached per
    (parent, column list)."""
    cache = qpn.__dict__.setdefault("_parent_maps", {})
    key = (pid, cols.tobytes())
    got = cache.get(key)
    if got is None:
        pd, okd = _positions(st["dec"], cols)
        pp, okp = _positions(st["par"], cols)
        got = cache[key] = np.where(okd, pd, np.where(okp, st["dec"].size + pp, -1)).astype(np.int32)
    return got


def parent_batches(qpn, items, eng, form: int, row_pad: int = ROW_PAD):
    """The record batches of `items` [(pid, [child Poly, ...])] made by eng.assemble_parent_nodes, grouped as batch_records
    groups them (form 0) or as it groups their free_equalities (form 1): one call per record shape.  The piece pool holds every
    distinct Poly once (by id) and goes up once, like the maps.  Returns (batches, rest): DeviceRecordBatch objects, and the
    positions of the items left to the host route -- a piece brings a column the parent does not read (node_record's second
    branch), no pieces, more than PARENT_SLOTS of them, or a stack beyond the entry's limits."""
    movers = up, down = _movers(eng)
    pool_of: Dict[int, int] = {}
    desc, cols_of, supp_of, eq_of, pA, pl, pu = [], [], [], [], [], [], []
    nrows = nwords = 0

    def piece_index(Pc: Poly) -> int:
        nonlocal nrows, nwords
        q = pool_of.get(id(Pc))
        if q is None:
            q = pool_of[id(Pc)] = len(desc)
            cols, A = Pc.local()
            supp = slice(None)
            if Pc._cols is None:
                # a dense Poly hands block() its columns as they are: a column of -0.0 alone (a flipped row's zeros) keeps its
                # signs there, so it comes along, outside the support node_record looks at
                supp = cols
                cols = np.nonzero(((Pc._A != 0) | np.signbit(Pc._A)).any(axis=0))[0].astype(np.int64)
                A = Pc._A[:, cols]
                supp = np.isin(cols, supp)
            supp_of.append(supp)
            desc.append((nrows, A.shape[0], A.shape[1], nwords))
            cols_of.append(cols); eq_of.append(int(np.count_nonzero(_is_eq(Pc.l, Pc.u))))
            pA.append(np.ascontiguousarray(A, dtype=np.float64).ravel()); pl.append(Pc.l); pu.append(Pc.u)
            nrows += A.shape[0]; nwords += A.size
        return q

    map_ids: Dict[tuple, int] = {}
    map_list: List[np.ndarray] = []
    plan, rest = {}, []
    groups: Dict[tuple, List[int]] = {}
    for i, (pid, ch) in enumerate(items):
        st = _static(qpn, pid)
        n0 = st["dec"].size
        if not ch or len(ch) > PARENT_SLOTS or not qpn.network_edges[pid]:
            rest.append(i)
            continue
        pcs = [piece_index(Pc) for Pc in ch]
        mps = [_parent_map(qpn, pid, st, cols_of[q]) for q in pcs]
        T = len(st["l"]) + sum(desc[q][1] for q in pcs)
        nE = (_parent_store(qpn, n0, eng)["base_eq"][pid] + sum(eq_of[q] for q in pcs)) if form else 0
        mi = T - nE
        mp = max(row_pad, -(-mi // row_pad) * row_pad) if mi else 0
        if any(np.any(mv[supp_of[q]] < 0) for q, mv in zip(pcs, mps)) or T > PARENT_MAX_ROWS or n0 + nE + mp > 1024:
            rest.append(i)
            continue
        mids = []
        for mv in mps:
            key = (pid, id(mv))
            if key not in map_ids:
                map_ids[key] = len(map_list); map_list.append(mv)
            mids.append(map_ids[key])
        plan[i] = (pcs, mids, mi)
        groups.setdefault((n0 + nE, mp, n0), []).append(i)
    batches = []
    if groups:
        pool = (up(np.array(desc, np.int32).reshape(-1, 4)), up(np.concatenate(pA + [np.zeros(0)])), up(np.concatenate(pl + [np.zeros(0)])),
                up(np.concatenate(pu + [np.zeros(0)])))
        moff = np.zeros(len(map_list) + 1, np.int32); moff[1:] = np.cumsum([mv.size for mv in map_list])
        maps = (up(moff), up(np.concatenate(map_list + [np.zeros(0, np.int32)]).astype(np.int32)))
    for (n, mp, n0), idx in sorted(groups.items()):
        S = _parent_store(qpn, n0, eng)
        sts = [_static(qpn, items[i][0]) for i in idx]
        p = max(1, max(s["par"].size for s in sts))
        nb = len(idx)
        parent_of = np.array([S["index"][items[i][0]] for i in idx], np.int32)
        piece_of = np.full((nb, PARENT_SLOTS), -1, np.int32); map_of = np.zeros((nb, PARENT_SLOTS), np.int32)
        for t, i in enumerate(idx):
            pcs, mids, _ = plan[i]
            piece_of[t, :len(pcs)] = pcs; map_of[t, :len(mids)] = mids
        out = eng.assemble_parent_nodes(form, n - n0, mp, p, *S["on"][1], *pool, *maps, up(parent_of), up(piece_of), up(map_of))
        err = np.asarray(down(out[7]))
        if err.any():
            raise RuntimeError(f"assemble_parent_nodes: bad items {np.nonzero(err)[0][:4].tolist()} (err {err[err != 0][:4].tolist()})")
        dec = np.stack([s["dec"] for s in sts]).astype(np.int64)
        par = np.full((nb, p), -1, dtype=np.int64)
        for t, s in enumerate(sts):
            par[t, :s["par"].size] = s["par"]
        batches.append(DeviceRecordBatch(idx, n, mp, p, n0, np.array([plan[i][2] for i in idx], dtype=np.int64), dec, par, out[:7], movers))
    return batches, rest


# ---------------------------------------------------------------------------------------------------------------------
# the level's pool split into connected components
# ---------------------------------------------------------------------------------------------------------------------
def components(qpn, players: Sequence[int], assign: Optional[Dict[int, Poly]] = None) -> List[List[int]]:
    """Connected components of the level's coupling graph.  Players i and j are coupled when they share a decision
    variable or when the KKT rows of one (Q_i[dvars_i, :], its base rows, its children's chosen pieces) read a decision
    variable of the other: those are the columns src/avi.jl:335-340 keeps in M.  Components come back as sorted id lists,
    ordered by their smallest id."""
    assign = assign or {}
    players = sorted(players)
    owner: Dict[int, int] = {}
    parent = {i: i for i in players}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    decs = {}
    for i in players:
        st = _static(qpn, i)
        decs[i] = st["dec"]
        for v in st["dec"].tolist():
            o = owner.get(v)
            if o is None:
                owner[v] = i
            else:
                ra, rb = find(o), find(i)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    for i in players:
        reads = [_static(qpn, i)["par"]]
        for j in sorted(qpn.network_edges[i]):
            if j in assign:
                reads.append(assign[j].support())
        for v in np.unique(np.concatenate(reads)).tolist():
            o = owner.get(v)
            if o is not None:
                ra, rb = find(o), find(i)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    comps: Dict[int, List[int]] = {}
    for i in players:
        comps.setdefault(find(i), []).append(i)
    return [sorted(c) for _, c in sorted(comps.items())]


def _pool_blocks_local(qpn, pool: List[int], assign: Dict[int, Poly]):
    """The numeric blocks of ONE multi-node component as qpn_assemble_pools takes them (avi.pool_blocks), with the
    component's own decision set and local parameters."""
    stat = {i: _static(qpn, i) for i in pool}
    dec = np.unique(np.concatenate([stat[i]["dec"] for i in pool]))
    cons = {i: list(stat[i]["base"]) + [assign[j] for j in sorted(qpn.network_edges[i]) if j in assign] for i in pool}
    reads = [stat[i]["par"] for i in pool] + [P.support() for i in pool for P in cons[i][len(stat[i]["base"]):]]
    par = np.setdiff1d(np.unique(np.concatenate(reads)), dec, assume_unique=True)
    pos = {int(d): k for k, d in enumerate(dec.tolist())}
    n_i = [stat[i]["dec"].size for i in pool]
    m_i = [sum(len(P) for P in cons[i]) for i in pool]
    dpos = [pos[int(d)] for i in pool for d in stat[i]["dec"].tolist()]
    f = {i: qpn.qps[i].f for i in pool}
    zero_d = np.zeros((0, dec.size)); zero_p = np.zeros((0, par.size))
    Qd = np.vstack([f[i].block(stat[i]["dec"], dec) for i in pool])
    Qp = np.vstack([f[i].block(stat[i]["dec"], par) for i in pool])
    qd = np.concatenate([stat[i]["qd"] for i in pool])
    Ad = np.vstack([zero_d] + [P.block(dec) for i in pool for P in cons[i]])
    Bp = np.vstack([zero_p] + [P.block(par) for i in pool for P in cons[i]])
    l = np.concatenate([np.zeros(0)] + [P.l for i in pool for P in cons[i]])
    u = np.concatenate([np.zeros(0)] + [P.u for i in pool for P in cons[i]])
    return dict(n_i=n_i, m_i=m_i, dpos=dpos, nd=int(dec.size), Qd=Qd, Qp=Qp, qd=qd, Ad=Ad, Bp=Bp, l=l, u=u, dec=dec, par=par)


# ---------------------------------------------------------------------------------------------------------------------
# warm start of a node sweep from the previous sweep's active set (QPN_AVI_FLAG_WARM_DUALS)
# ---------------------------------------------------------------------------------------------------------------------
# False: every sweep of solve_level solves its nodes from cold duals (the code as it was).  True: solve_level keeps the last z of
# every resident childless batch where the engine computes and hands it to the next sweep's solve as the hint; inner nodes and
# pools stay cold.  The hint is passed for any shape: the engine honours it for n, m <= 32, and for large resident batches
# (64 < n <= 256, m <= 256, symmetric Qd) once the engine's option OPT_WARM_BIG is set; everywhere else it is ignored.
WARM_DUALS_ROUTE = False
# The mid-size classes (n, m <= 128, one of them > 32) take the hint per handle (Nodes.set_warm).  True, together
# with WARM_DUALS_ROUTE: the resident childless batches opt in once, when their handle is made.  False: everything as without it.
WARM_DUALS_MID = False
WARM_CHECK_TOL, WARM_PIV_TOL, WARM_COMP_TOL = 1e-6, 1e-11, 1e-2     # qpn_avi_default_opts
# Sweeps over a part of a resident childless batch (Nodes.solve_subset).  False: solve_level solves every record of
# the batch and keeps the rows of the players asked for (the code as it was).  True, with WARM_DUALS_ROUTE off and a handle that
# has solve_subset: a sweep that leaves records of a batch out -- the players of settled components -- hands over only the
# records asked for, their rows of w, and gets only their rows back.  x_opt is the same bit for bit.
SUBSET_SWEEP_ROUTE = False
# The accept gate over a part of a resident childless batch (Nodes.verify_subset).  False: process_level verifies
# every node of an all-leaf level in every sweep (the code as it was).  True, with a handle that has verify_subset: the players
# whose result the memo already holds are left out of the verify call -- none is made when every player is a hit, the full one
# when none is.  process_level returns the same list, value for value.
SUBSET_VERIFY_ROUTE = False


def _eliminate(M, rhs, piv_tol):
    """M y = rhs by Gaussian elimination with partial pivoting, rhs [rows, columns] -> y, or None when a pivot is below piv_tol
    (or is no number)."""
    M = np.array(M, dtype=np.float64); y = np.array(rhs, dtype=np.float64)
    k = M.shape[0]
    for j in range(k):
        col = np.abs(M[j:, j])
        if not np.all(np.isfinite(col)):
            return None
        pr = j + int(np.argmax(col))
        if not abs(M[pr, j]) >= piv_tol:
            return None
        if pr != j:
            M[[j, pr]] = M[[pr, j]]; y[[j, pr]] = y[[pr, j]]
        f = M[j + 1:, j] / M[j, j]
        M[j + 1:, j + 1:] -= np.outer(f, M[j, j + 1:])
        y[j + 1:] -= np.outer(f, y[j])
    for i in range(k - 1, -1, -1):
        y[i] = (y[i] - M[i, i + 1:] @ y[i + 1:]) / M[i, i]
    return y


def node_postcheck(z, r, l, u, n, check_tol=WARM_CHECK_TOL, comp_tol=WARM_COMP_TOL):
    """The post-check of a node solve on z = [x; lam] and r = M z + q (check_avi_solution, src/avi.jl:148-156, on the rows
    [free STD x n | GAVI x m] with the bounds l, u of the m constraint rows), the natural-map residual and the active-set masks of
    src/avi_solutions.jl:511-562 (x rows: bit c - 1 for code c, constraint rows: bit c + 3) -> (bad, resid, active).
    The numpy twin of QPN_ROW_POSTCHECK (csrc/qpn_internal.h: QPN_ROW_VIOLATIONS, QPN_ROW_RESIDUAL, QPN_ROW_MASK with qpn_approx),
    the one row post-check of every solver kernel, row for row; bad is "any violation", resid the maximum over the rows.
    tests/test_postcheck_host.py holds the two together."""
    z = np.asarray(z, dtype=np.float64); r = np.asarray(r, dtype=np.float64)
    N = z.size
    lk = np.concatenate([np.full(n, -INF), l]); uk = np.concatenate([np.full(n, INF), u])
    gk = np.arange(N) >= n
    pp = np.where(gk, r, z); dv = np.where(gk, z, r)
    with np.errstate(invalid="ignore"):
        bad = ((dv > check_tol) & (np.abs(pp - lk) > check_tol)) | ((dv < -check_tol) & (np.abs(pp - uk) > check_tol)) \
            | (pp - lk < -check_tol) | (pp - uk > check_tol) | np.isnan(pp) | np.isnan(dv)
        nres = np.abs(pp - np.minimum(np.maximum(pp - dv, lk), uk))
        nres = np.where(np.isnan(nres), INF, nres)
        approx = lambda x, y: (x == y) | (np.abs(x - y) <= comp_tol)
        mask = np.where(approx(lk, uk), 8,
                        1 * (approx(pp, lk) & (dv >= -comp_tol)) + 2 * ((lk - comp_tol <= pp) & (pp <= uk + comp_tol) & (np.abs(dv) <= comp_tol))
                        + 4 * (approx(pp, uk) & (dv <= comp_tol))).astype(np.uint8)
    mask = np.where(gk, mask << 4, mask).astype(np.uint8)
    return bool(bad.any()), float(nres.max()) if N else 0.0, mask


WARM_MID_LDS, WARM_MID_FIXED = 160 * 1024, 15648     # kWarmMidLds, kWarmMidFixed (csrc/qpn_internal.h)


def warm_mid_fits(n, k):
    """warm_mid_fits of csrc/qpn_internal.h restated: does the warm kernel of the mid-size classes (csrc/qpn_warm_mid.hip) hold a
    hint of k rows on a node with n variables -- A_act (k x n) and W | h (n x (k + 1)), both with odd row strides, beside the
    fixed part of its LDS?  A pure function of (n, k), monotone in k."""
    n, k = int(n), int(k)
    return 0 <= k <= n and 8 * (k * (n | 1) + n * ((k + 1) | 1)) + WARM_MID_FIXED <= WARM_MID_LDS


def warm_nodes_host(records, w, z_prev, opts=None, fits=None):
    """Numpy twin of the warm kernels (csrc/qpn_warm.hip, csrc/qpn_warm_mid.hip).  records = (Qc, Rc, qd, Ac, Bc, l, u) in the ABI layout, w (p,) or
    (batch, p), z_prev [batch, n + m]: its multipliers name the hint (side +1 where lambda > 0, -1 where < 0, 0 otherwise).
    Per node the linear KKT system of the hinted rows, [[Qd, -A_act'], [A_act, 0]] [x; lam_act] = [-(qd + R w); bound_act -
    B_act w], by block elimination through Qd and the k x k Schur block (partial pivoting, fp64).

    THE ACCEPT RULE -- a node is accepted only if all of these hold:
      every hinted multiplier is finite and its row has a finite bound on its side;  k <= n;  no pivot of the two eliminations
      is below piv_tol;  every lam_act carries its side's sign (lam_act * side > 0);  the post-check of the cold solve passes
      (check_tol, on the original blocks);  with fits= (a predicate of (n, k): warm_mid_fits for the mid-size kernel), fits(n, k).
    -> dict(accepted [batch] bool, z, status, resid, pivots, active): for an accepted node its point, status 1 (SUCCESS), the
    natural-map residual, pivots 0 and the masks (comp_tol); a declined node keeps z_prev's row, status 0, resid NaN, pivots -1,
    active 0 -- the caller solves it cold."""
    Qc, Rc, qd, Ac, Bc, l, u = (np.asarray(a, dtype=np.float64) for a in records)
    check_tol = getattr(opts, "check_tol", WARM_CHECK_TOL); piv_tol = getattr(opts, "piv_tol", WARM_PIV_TOL)
    comp_tol = getattr(opts, "comp_tol", WARM_COMP_TOL)
    batch, n = qd.shape
    m = l.shape[1]
    w = np.asarray(w, dtype=np.float64)
    z_prev = np.asarray(z_prev, dtype=np.float64).reshape(batch, n + m)
    out = dict(accepted=np.zeros(batch, bool), z=z_prev.copy(), status=np.zeros(batch, np.int32), resid=np.full(batch, np.nan),
               pivots=np.full(batch, -1, np.int32), active=np.zeros((batch, n + m), np.uint8))
    for b in range(batch):
        Q, R, A, B = Qc[b].T, Rc[b].T.reshape(n, -1), Ac[b].T.reshape(m, n), Bc[b].T.reshape(m, -1)
        wb = w if w.ndim == 1 else w[b]
        lam0 = z_prev[b, n:]
        if not np.all(np.isfinite(lam0)):
            continue
        side = np.sign(lam0).astype(np.int64)
        rows = np.flatnonzero(side)
        k = rows.size
        bound = np.where(side > 0, l[b], u[b])[rows]
        if k > n or not np.all(np.isfinite(bound)):
            continue
        if fits is not None and not fits(n, k):
            continue
        q = qd[b] + R @ wb
        c = B @ wb
        Aa = A[rows]
        W = _eliminate(Q, np.column_stack([Aa.T, -q]), piv_tol)            # [Qd^-1 A_act' | h]
        if W is None:
            continue
        lam = np.zeros(0)
        if k:
            lam = _eliminate(Aa @ W[:, :k], (bound - c[rows] - Aa @ W[:, k])[:, None], piv_tol)
            if lam is None:
                continue
            lam = lam[:, 0]
            if not np.all(lam * side[rows] > 0):
                continue
        z = np.zeros(n + m)
        z[:n] = W[:, k] + W[:, :k] @ lam
        z[n + rows] = lam
        r = np.concatenate([q + Q @ z[:n] - A.T @ z[n:], c + A @ z[:n]])
        bad, resid, mask = node_postcheck(z, r, l[b], u[b], n, check_tol, comp_tol)
        if bad:
            continue
        out["accepted"][b] = True
        out["z"][b] = z; out["status"][b] = 1; out["resid"][b] = resid; out["pivots"][b] = 0; out["active"][b] = mask
    return out


# block principal pivoting of the large class (csrc/qpn_avi_schur_big.hip: schur_big_bpp) and its warm start
BPP_KMAX, BPP_MAX_IT, BPP_PIV_REL = 112, 30, 1e-13


def _bpp_factor_ok(SAA):
    """The failure test of the kernel's tile Cholesky (csrc/qpn_tile_chol.h) on the lower triangle of SAA: every pivot has to lie
    above 1e-13 max(1, first diagonal entry of its 16 x 16 tile, as updated by the tile columns before it)."""
    L = np.tril(np.array(SAA, dtype=np.float64))
    k = L.shape[0]
    d0 = 1.0
    for j in range(k):
        if j % 16 == 0:
            d0 = max(1.0, abs(L[j, j]))
        pv = L[j, j]
        if not pv > BPP_PIV_REL * d0:
            return False
        L[j:, j] /= np.sqrt(pv)
        col = L[j + 1:, j]
        L[j + 1:, j + 1:] -= np.tril(np.outer(col, col))
    return True


def warm_big_host(S, c, l, u, lam_hint=None):
    """Numpy twin of Stage B of a large symmetric node, schur_big_bpp, on its Schur problem: find lam with s = S lam + c in
    [l, u], lam_i >= 0 only where s_i = l_i, <= 0 only where s_i = u_i (S [m, m] symmetric, m <= 256).

    THE SEED RULE (lam_hint given: QPN_OPT_WARM_BIG with QPN_AVI_FLAG_WARM_DUALS) -- row i starts at l_i if lam_hint_i > 0 and l_i
    is finite, at u_i if lam_hint_i < 0 and u_i is finite, and inactive otherwise (NaN, +-0).  THE CAP RULE -- a seed of no row or
    of more than BPP_KMAX rows is dropped: the cold start alone runs.  lam_hint = None is the cold start: the rows violated at
    lam = 0, the BPP_KMAX most violated ones when there are more.  THE ROUNDS -- with A the rows at a bound, lam_A solves
    S_AA lam_A = t_A - c_A, lam = 0 elsewhere, s = c + S(:, A) lam_A; rows of A whose multiplier has the wrong sign leave, free
    rows outside their interval enter (lowest index first while A has room), until no pair is violated (tolerances 1e-10 x
    scale); the count of violated pairs has to reach a new minimum within three rounds, otherwise only the violated pair of the
    highest index is switched (Murty).  An attempt fails on a pivot of the Cholesky factorisation under its threshold or after
    BPP_MAX_IT rounds.  THE RESTART -- a failed seeded attempt is followed by one cold attempt.  The systems are solved with S_AA
    itself (the kernel factors the lower triangle and refines once with the rows of S on the final set).

    -> dict(lam [m], side [m] int8 (0 free, 1 at l, 2 at u), rounds, switched, finished, seeded, restarted): rounds and switched
    (the complementarity pairs switched after the start) count over both attempts; finished = False is the kernel's
    BPP_NOT_SOLVED (an equality row, or every attempt failed) and leaves lam zero."""
    S = np.asarray(S, dtype=np.float64); c = np.asarray(c, dtype=np.float64)
    l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    m = c.size
    out = dict(lam=np.zeros(m), side=np.zeros(m, np.int8), rounds=0, switched=0, finished=False, seeded=False, restarted=False)
    if m < 1 or m > 256 or np.any(l == u):
        return out
    scale = max(1.0, np.max(np.abs(c)), np.max(np.abs(l[l > -INF]), initial=0.0), np.max(np.abs(u[u < INF]), initial=0.0))
    tol_s = 1e-10 * scale

    def cold():
        v0 = np.maximum(l - c, c - u)
        viol = v0 > tol_s
        if viol.sum() > BPP_KMAX:
            lo_, hi_ = tol_s, float(v0.max())
            for _ in range(12):
                mid = 0.5 * (lo_ + hi_)
                if (v0 > mid).sum() > BPP_KMAX:
                    lo_ = mid
                else:
                    hi_ = mid
            viol = v0 > hi_
        return np.where(viol, np.where(c < l, 1, 2), 0).astype(np.int8)

    starts = [cold]
    if lam_hint is not None:
        h = np.asarray(lam_hint, dtype=np.float64).reshape(m)
        with np.errstate(invalid="ignore"):
            seed = np.where((h > 0) & (l > -INF), 1, np.where((h < 0) & (u < INF), 2, 0)).astype(np.int8)
        if 1 <= np.count_nonzero(seed) <= BPP_KMAX:
            starts = [lambda: seed.copy(), cold]
            out["seeded"] = True
    for attempt, start in enumerate(starts):
        st = start()
        out["restarted"] = attempt > 0
        nbest, patience = m + 1, 3
        for _ in range(BPP_MAX_IT):
            out["rounds"] += 1
            A = np.flatnonzero(st)
            k = A.size
            lam = np.zeros(m)
            if k:
                SAA = S[np.ix_(A, A)]
                if not _bpp_factor_ok(SAA):
                    break
                lam[A] = np.linalg.solve(SAA, np.where(st[A] == 1, l[A], u[A]) - c[A])
            s = c + S[A].T @ lam[A]                             # (rows A of S: the kernel reads the column block this way)
            s = np.where(st == 1, l, np.where(st == 2, u, s))
            tol_l = 1e-10 * max(1.0, np.max(np.abs(lam)))
            bad = ((st == 1) & (lam < -tol_l)) | ((st == 2) & (lam > tol_l)) | ((st == 0) & ((s < l - tol_s) | (s > u + tol_s)))
            nb = int(bad.sum())
            if nb == 0:
                out.update(lam=lam, side=st, finished=True)
                return out
            flip = bad
            if nb < nbest:
                nbest, patience = nb, 3
            elif patience > 0:
                patience -= 1
            else:
                flip = np.zeros(m, bool); flip[np.flatnonzero(bad)[-1]] = True
            leave = flip & (st != 0)
            enter = np.flatnonzero(flip & (st == 0))
            room = BPP_KMAX - (k - int(leave.sum()))
            st = st.copy()
            st[leave] = 0
            enter = enter[:max(room, 0)]
            st[enter] = np.where(s[enter] < l[enter], 1, 2)
            out["switched"] += int(leave.sum()) + enter.size
    return out


# ---------------------------------------------------------------------------------------------------------------------
# solve_qep for a level: src/avi.jl:382-444 over the components
# ---------------------------------------------------------------------------------------------------------------------
def _leaf_batches(qpn, players, engine, free_eq=False):
    """Record batches of the childless nodes among `players`: they depend on the net alone, so they are built once per
    (net, player set) and keep a resident handle.  free_eq: the solve's form of the records (free_equalities)."""
    cache = qpn.__dict__.setdefault("_leaf_batches", {})
    key = (tuple(players), bool(free_eq))
    got = cache.get(key)
    if got is None:
        recs = [node_record(qpn, i) for i in players]
        if free_eq:
            recs = [free_equalities(r) for r in recs]
        got = cache[key] = (recs, batch_records(recs))
    return got


def _warm_sweep(b, h, eng, w):
    """One sweep of a resident childless batch under WARM_DUALS_ROUTE: the outputs of the batch's last sweep stay where the
    engine computes (b.warm_out, kept per handle), and their z goes into this sweep as the hint -- in place, the solution
    overwrites it.  The first sweep of a handle has no hint and is the cold call."""
    up, down = _movers(eng)
    kept = getattr(b, "warm_out", None)
    if kept is not None and kept[0] is h:
        out = h.solve(up(w), out=kept[1], warm=kept[1]["z"])
    else:
        out = h.solve(up(w), want=("z", "resid", "pivots"))
    b.warm_out = (h, out)
    return dict(status=down(out["status"]), z=down(out["z"]))


def solve_level(qpn, players: Sequence[int], x, assign: Optional[Dict[int, Poly]] = None, engine=None, reference_form=False,
                settled: Optional[set] = None):
    """solve_qep (src/avi.jl:382-444) for a whole level: x_opt with every component's decision block replaced by the
    solution of its AVI.  Raises avi.AVISolveError when any component's solve does not end in SUCCESS (:426).

    `settled` (ids of players verify_solution has just accepted): a component ALL of whose players are settled is left where it
    is.  The reference re-solves it with the rest of the level, under its children's FIRST pieces (src/algorithm.jl:54, :95); the
    point passes verify_solution under every piece combination, so that solve returns it again -- up to the 1e-4 band of the
    accept tests, inside which two pieces' exact minimisers can differ: re-solved sweep after sweep while OTHER components are
    still moving, such a component jumps between them and the level ends in "Cycling detected", although the component on its
    own (or the net sharded by cluster, sharding.solve_sharded) is done.  With the split into components the engine knows
    which blocks of the level's AVI are already at rest."""
    from .avi import AVISolveError, StatusCode, _eng
    from .engine import colmajor
    eng = _eng(engine)
    assign = assign or {}
    x = np.asarray(x, dtype=np.float64)
    x_opt = x.copy()
    comps = components(qpn, players, assign)
    if settled:
        comps = [c for c in comps if not all(i in settled for i in c)]
    singles = [c[0] for c in comps if len(c) == 1]
    multis = [c for c in comps if len(c) > 1]
    bad = []
    # ---- single-node components: node records, one call per record shape
    leaf = [i for i in singles if not qpn.network_edges[i]]
    inner = [i for i in singles if qpn.network_edges[i]]
    work = []
    take = None
    if leaf and not reference_form:
        # ONE resident batch per level for all its childless players (built once per net): every record is solved -- one launch
        # whatever the subset -- and only the players asked for are written back (a batch per subset would upload a new copy of
        # the records whenever the set of unsettled players changes)
        universe = [i for i in sorted(players) if not qpn.network_edges[i]]
        recs_u, batches_u = _leaf_batches(qpn, universe, eng, free_eq=True)
        wanted = set(leaf)
        take = {id(b): np.array([recs_u[i]["pid"] in wanted for i in b.where]) for b in batches_u}
        work += [(b, True) for b in batches_u if take[id(b)].any()]
    elif leaf:
        inner = sorted(inner + leaf)
    if inner and not reference_form and _parent_route(eng):
        # the records are made on the device (parent_batches); the few items it leaves go the host way below
        its = [(i, [assign[j] for j in sorted(qpn.network_edges[i]) if j in assign]) for i in inner]
        dev_batches, rest = parent_batches(qpn, its, eng, 1)
        work += [(b, False) for b in dev_batches]
        work += [(b, False) for b in batch_records([free_equalities(node_record(qpn, *its[t])) for t in rest])]
    elif inner:
        recs = [node_record(qpn, i, [assign[j] for j in sorted(qpn.network_edges[i]) if j in assign]) for i in inner]
        if reference_form:
            work += [(r, None) for r in recs]
        else:
            work += [(b, False) for b in batch_records([free_equalities(r) for r in recs])]
    for item, static in work:
        if static is None:
            _solve_single_reference_form(item, x, x_opt, eng, bad)
            continue
        b = item
        xd, w = b.gather(x)
        z0 = np.zeros((len(b), b.n + b.m)); z0[:, :b.nx] = xd                       # duals cold, :404
        h = b.resident(eng, WARM_DUALS_ROUTE and WARM_DUALS_MID) if static else None
        sel = take[id(b)] if (static and take is not None) else np.ones(len(b), bool)
        rows = np.flatnonzero(sel)                       # the records whose players are written back
        if SUBSET_SWEEP_ROUTE and not WARM_DUALS_ROUTE and h is not None and hasattr(h, "solve_subset") and not sel.all():
            # only the records asked for go to the engine: slot s of the answer belongs to record rows[s]
            res = h.solve_subset(rows.astype(np.int32), w[rows], want=("z", "resid", "pivots"))
            st = np.asarray(res["status"])
            z = np.asarray(res["z"])
        else:
            if h is not None and WARM_DUALS_ROUTE:
                res = _warm_sweep(b, h, eng, w)
            elif h is not None:
                res = h.solve(w, want=("z", "resid", "pivots"))
            elif isinstance(b, DeviceRecordBatch):
                res = b.solve(eng, w, z0)
            else:
                res = eng.solve_nodes(b.Qc, b.Rc, b.qd, b.Ac, b.Bc, b.l, b.u, w, z0=z0)
            st = np.asarray(res["status"])[rows]
            z = np.asarray(res["z"])[rows]
        if np.any(st != StatusCode.SUCCESS):
            k = int(np.nonzero(st != StatusCode.SUCCESS)[0][0])
            bad.append((int(b.dec[rows[k]][0]), int(st[k])))
        x_opt[b.dec[rows].ravel()] = z[:, :b.nx].ravel()                             # :440-443
    # ---- multi-node components: pool AVIs, one assemble + one solve per pool shape
    if multis:
        blocks = [_pool_blocks_local(qpn, c, assign) for c in multis]
        sig: Dict[tuple, List[int]] = {}
        for k, bl in enumerate(blocks):
            disjoint = sum(bl["n_i"]) == bl["nd"]
            form = "reference" if (reference_form or not disjoint) else "reduced"
            sig.setdefault((tuple(bl["n_i"]), tuple(bl["m_i"]), tuple(bl["dpos"]), bl["nd"], bl["par"].size, form), []).append(k)
        for key, ks in sorted(sig.items()):
            form = key[-1]
            b0 = blocks[ks[0]]
            p = max(1, b0["par"].size)
            pad = lambda M: np.hstack([M, np.zeros((M.shape[0], p - M.shape[1]))]) if M.shape[1] < p else M
            stack = lambda name: np.stack([colmajor(pad(blocks[k][name]) if name in ("Qp", "Bp") else blocks[k][name]) for k in ks])
            w = np.stack([np.concatenate([x[blocks[k]["par"]], np.zeros(p - blocks[k]["par"].size)]) for k in ks])
            Mc, q, lo, hi, kind = eng.assemble_pools(b0["n_i"], b0["m_i"], b0["dpos"], b0["nd"], stack("Qd"), stack("Qp"),
                                                     np.stack([blocks[k]["qd"] for k in ks]), stack("Ad"), stack("Bp"),
                                                     np.stack([blocks[k]["l"] for k in ks]), np.stack([blocks[k]["u"] for k in ks]),
                                                     w, form=form, share_M=False)
            q = np.asarray(q); Nn = q.shape[-1]
            nd = b0["nd"]
            z0 = np.zeros((len(ks), Nn))
            for t, k in enumerate(ks):
                z0[t, :nd] = x[blocks[k]["dec"]]
                if form == "reference":
                    sm = len(blocks[k]["l"])
                    if sm:                                                          # z0s = [z0; A z0 + B w], :107-108
                        z0[t, Nn - sm:] = blocks[k]["Ad"] @ x[blocks[k]["dec"]] + blocks[k]["Bp"] @ x[blocks[k]["par"]]
            res = eng.solve_avi_batch(np.asarray(Mc).reshape(len(ks), Nn, Nn), q.reshape(len(ks), Nn), np.asarray(lo).reshape(len(ks), Nn),
                                      np.asarray(hi).reshape(len(ks), Nn), z0=z0, kind=np.asarray(kind).reshape(len(ks), Nn))
            st = np.asarray(res["status"]); z = np.asarray(res["z"])
            for t, k in enumerate(ks):
                if int(st[t]) != StatusCode.SUCCESS:
                    bad.append((multis[k], int(st[t])))
                x_opt[blocks[k]["dec"]] = z[t, :nd]
    if bad:
        raise AVISolveError(f"AVI solve error. This might be because one of the qps {list(players)} is unbounded or "
                            f"ill-conditioned. (first failures: {bad[:4]})")
    return x_opt


def _solve_single_reference_form(rec, x, x_opt, eng, bad):
    """One single-node component through the reference's own AVI (xi and slack blocks, convert(): src/avi.jl:113-128) --
    the parity route of solve_qep(reference_form=True)."""
    from .avi import GAVI, StatusCode, solve_gavi
    n, m = rec["dec"].size, len(rec["l"])
    # z = [x_d; xi; lambda], rows [sum xi = 0 ; KKT rows], A = [Ad 0 0]
    M = np.block([[np.zeros((n, n)), np.eye(n), np.zeros((n, m))], [rec["Qd"], np.zeros((n, n)), -rec["Ad"].T]])
    Nn = np.vstack([np.zeros((n, rec["par"].size)), rec["R"]])
    o = np.concatenate([np.zeros(n), rec["qd"]])
    A = np.hstack([rec["Ad"], np.zeros((m, n + m))])
    g = GAVI(M, Nn, o, np.full(2 * n, -INF), np.full(2 * n, INF), A, rec["B"], rec["l"], rec["u"])
    z0 = np.zeros(2 * n + m); z0[:n] = x[rec["dec"]]
    z, status, _ = solve_gavi(g, z0, x[rec["par"]], engine=eng, reference_form=True)
    if status != StatusCode.SUCCESS:
        bad.append((rec["pid"], int(status)))
    x_opt[rec["dec"]] = z[:n]


# ---------------------------------------------------------------------------------------------------------------------
# process_qp for a level: src/algorithm.jl:44-52 over src/qp_processing.jl:151-241
# ---------------------------------------------------------------------------------------------------------------------
_VERIFY_MSGS = {0: "Current point is infeasible when using tolerance {tol}.", 1: "Current point is suboptimal",
                4: "Current point is suboptimal (via QP).", 5: "Solving for duals failed."}


def verify_items(qpn, items, x, engine, tol=1e-4, check_convexity=False, only=None):
    """verify_solution (src/qp_processing.jl:57-149) for MANY (node, child pieces) items: one qpn_verify_nodes call per
    record shape.  items: list of (pid, [child Poly, ...]).  Returns (records, batches, one result dict per item).
    check_convexity runs check_qp_convexity (:69) on every item first: qp_processing.check_convexity_items, which raises
    NonConvexQPError for the first non-convex item.
    only (SUBSET_VERIFY_ROUTE; childless items on a handle that has verify_subset): the positions in `items` to verify.  The
    other items' results stay None, and a batch none of whose items is asked for makes no call."""
    eng = engine
    if check_convexity:
        from .qp_processing import check_convexity_items
        check_convexity_items(qpn, items, eng)
    leaf_ids = tuple(pid for pid, ch in items if not ch)
    all_leaf = len(leaf_ids) == len(items)
    if all_leaf:
        recs, batches = _leaf_batches(qpn, list(leaf_ids), eng)
    elif _parent_route(eng):
        # the records are made on the device (parent_batches): the host keeps an item's pid; the items left over go the host way
        batches, rest = parent_batches(qpn, items, eng, 0)
        recs = [dict(pid=pid) for pid, _ in items]
        for i in rest:
            recs[i] = node_record(qpn, *items[i])
        host_batches = batch_records([recs[i] for i in rest])
        for b in host_batches:
            b.where = [rest[k] for k in b.where]
        batches = batches + host_batches
    else:
        recs = [node_record(qpn, pid, ch) for pid, ch in items]
        batches = batch_records(recs)
    out = [None] * len(items)
    asked = None if only is None else set(only)
    for b in batches:
        xd, w = b.gather(x)
        h = b.resident(eng) if all_leaf else None
        # the rows of the batch to verify: all of them, or under `only` those asked for (compact call, compact outputs)
        rows = np.arange(len(b.where), dtype=np.int32)
        if only is not None and h is not None and hasattr(h, "verify_subset"):
            rows = rows[[i in asked for i in b.where]]
        if rows.size == 0:
            sol, lam, path = (), np.zeros((0, b.m)), ()
        elif rows.size < len(b.where):
            sol, lam, path = h.verify_subset(rows, xd[rows], w[rows], tol=tol)
        elif h is not None:
            sol, lam, path = h.verify(xd, w, tol=tol)
        elif isinstance(b, DeviceRecordBatch):
            sol, lam, path = b.verify(eng, xd, w, tol)
        else:
            sol, lam, path = eng.verify_nodes(b.Qc, b.Rc, b.qd, b.Ac, b.Bc, b.l, b.u, xd, w, tol=tol)
        sol = np.asarray(sol); lam = np.asarray(lam); path = np.asarray(path)
        for s, k in enumerate(rows):
            pth = int(path[s]); ok = bool(sol[s]); mi = int(b.m_true[k])
            out[b.where[k]] = dict(solution=ok, lam=(lam[s, :mi].copy() if pth in (1, 2, 3, 4) else None),
                                   e=None if ok else _VERIFY_MSGS.get(pth, "").format(tol=tol), path=pth)
        if rows.size < len(b.where):                                # (the rows left out keep a zero row)
            lam_r, lam = lam, np.zeros((len(b.where), lam.shape[1]))
            lam[rows] = lam_r
        b.last = dict(xd=xd, w=w, lam=lam)
    return recs, batches, out


# The uncapped route (QPNetOptions.max_pieces = None) enumerates every recipe of a node, as the reference does
# (src/qp_processing.jl:193-198, :231 -> all_Ks, src/avi_solutions.jl:200-215).  A node with more recipes than this is refused:
# the route never truncates silently.
MAX_RECIPES = 1 << 24
# The recipes of a record batch go through the device in chunks whose reduced pieces, their workspace and the finished store
# stay under this many bytes.
CHUNK_BYTES = 256 << 20


def _piece_masks(b, sel, rets, want, tol, eng):
    """The code sets of every wanted record of a batch at (x, lambda) (comp_indices, src/avi_solutions.jl:511-562, refined by
    _refine_row_codes) and the size of each one's recipe product."""
    n, m = b.n, b.m
    xd, w = b.last["xd"], b.last["w"]
    lam = np.zeros((len(b), m))
    for k, i in enumerate(b.where):
        if want[i]:
            lam[k, :b.m_true[k]] = rets[i]["lam"]
    # the node's own GAVI at z = [x_d; lambda], w = x_p (src/avi.jl:447-477): r1 = Qd x + R w + qd - Ad' lambda, s = Ad x + B w
    r1 = np.einsum("bji,bj->bi", b.Qc, xd) + np.einsum("bji,bj->bi", b.Rc, w) + b.qd - np.einsum("bij,bj->bi", b.Ac, lam)
    s = np.einsum("bji,bj->bi", b.Ac, xd) + np.einsum("bji,bj->bi", b.Bc, w)
    free_lo = np.full((len(sel), n), -INF); free_hi = np.full((len(sel), n), INF)
    m1 = np.asarray(eng.comp_indices(xd[sel], r1[sel], free_lo, free_hi, tol=tol, shift=0))
    m2 = np.asarray(eng.comp_indices(s[sel], lam[sel], b.l[sel], b.u[sel], tol=tol, shift=4)) if m else np.zeros((len(sel), 0), np.uint8)
    for t, k in enumerate(sel):                          # inert padding rows: l = -inf, u = inf, lambda = 0 -> code 6 only
        m2[t, b.m_true[k]:] = 1 << 5
    if m:
        m2 = _refine_row_codes(m2, s[sel], lam[sel], b.l[sel], b.u[sel], CODE_TOL)
    masks = np.concatenate([m1, m2], axis=1).astype(np.uint8)
    ok = ~np.any(masks == 0, axis=1)                     # a zero mask: (x, lambda) is no solution of the GAVI at this tolerance
    pop = np.array([[bin(int(v)).count("1") for v in row] for row in masks], dtype=np.float64)
    total = np.where(ok, np.prod(np.maximum(pop, 1.0), axis=1), 0.0)
    return masks, total


def _colsel(b, k):
    """A record's piece columns [x_d; x_p present] in ascending global order, and where each sits among Ar's n + p columns."""
    pk = np.nonzero(b.par[k] >= 0)[0]
    cols = np.concatenate([b.dec[k], b.par[k][pk]])
    order = np.argsort(cols, kind="stable")
    return cols[order], np.concatenate([np.arange(b.n), b.n + pk])[order]


def _finish_host(Ar, lr, ur, rows, plain, take_k, xk, probe):
    """Pieces `plain` of one record (reduced_pieces' output) over the record's columns take_k in ascending global order,
    normalised as Poly does (src/sets.jl:76-89: 1e-8 drop, leading coefficient +1); the point's worst violation per piece (xk:
    the point on those columns); _dedupe's quick merge test; the 6-digit rounded keys.  Returns (worst, A3 [pieces, Rmax, cols],
    L2, U2 [pieces, Rmax], merge, A6, LU6 [pieces, 2 Rmax]).  qpn_finish_pieces does the same operations in the same order."""
    Rmax = Ar.shape[2]
    # all of the record's pieces at once: rows over the columns in ascending order, normalised as Poly does
    # (src/sets.jl:76-89: 1e-8 drop, leading coefficient +1), the point's worst violation per piece
    A3 = np.ascontiguousarray(np.swapaxes(Ar[plain][:, take_k, :], 1, 2))        # [pieces, Rmax, columns]
    L2 = lr[plain].astype(np.float64, copy=True); U2 = ur[plain].astype(np.float64, copy=True)
    # (first to unit largest coefficient: the rows come out of the elimination at any scale -- a stationarity row of
    #  size 1e-4 whose 1e-8 entry is dropped, then divided by a leading coefficient of 1e-6, misses its own point by
    #  7e-3, and the parent calls the point infeasible: one pair in 5 000 at n = m = 32 cycled on exactly that)
    big = np.max(np.abs(A3), axis=2)
    sc = np.where(big > 0.0, 1.0 / np.where(big > 0.0, big, 1.0), 1.0)
    A3 *= sc[..., None]
    with np.errstate(invalid="ignore"):
        L2 = L2 * sc; U2 = U2 * sc
    A3[np.abs(A3) < 1e-8] = 0.0
    nzm = A3 != 0
    has = nzm.any(axis=2)
    lead = np.where(has, np.take_along_axis(A3, nzm.argmax(axis=2)[..., None], axis=2)[..., 0], 1.0)
    nrm = np.abs(lead); neg = has & (lead < 0)
    A3 /= np.where(neg, -nrm, nrm)[..., None]
    with np.errstate(invalid="ignore"):
        ln, un = L2 / nrm, U2 / nrm
    L2 = np.where(neg, -un, ln); U2 = np.where(neg, -ln, un)
    ax = A3 @ xk
    live = has & (np.arange(Rmax)[None, :] < rows[plain][:, None])
    viol = np.where(live, np.maximum(L2 - ax, ax - U2), 0.0)
    worst = np.max(viol, axis=1, initial=0.0)
    # _dedupe's own quick test (equal normals project equally on a random vector; all-zero rows) for all pieces at once:
    # the few that have something to merge go through it, the others are taken as they are
    valid = np.arange(Rmax)[None, :] < rows[plain][:, None]
    with np.errstate(invalid="ignore"):
        hs = np.sort(np.where(valid, A3 @ probe, np.inf), axis=1)
        close = np.diff(hs, axis=1) <= 1e-7 * (1.0 + np.abs(hs[:, 1:]))
    merge = np.any(close & np.isfinite(hs[:, 1:]), axis=1) | np.any(valid & ~has, axis=1)
    A6 = np.round(A3, 6) + 0.0                      # (the keys of the node's piece SET, rounded once for all pieces)
    LU6 = np.round(np.concatenate([L2, U2], axis=1), 6)
    return worst, A3, L2, U2, merge, A6, LU6


_HG, _HC1, _HC2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def _fin64(z):
    z = (z ^ (z >> np.uint64(30))) * _HC1
    z = (z ^ (z >> np.uint64(27))) * _HC2
    return z ^ (z >> np.uint64(31))


def _key_hash(A6, L6, U6, r):
    """64 bits of the keys of many pieces, as qpn_finish_pieces computes them: A6 [pieces, R, cols] the rounded rows, L6, U6
    [pieces, R] the rounded bounds, r [pieces] the valid rows.  Word j of a key (the r x cols rows row-major, then the r lower and
    the r upper bounds) adds fin64(bits + (j + 1) G); the sum (mod 2^64) is mixed once more with r."""
    P, R, nc = A6.shape
    r = np.asarray(r, dtype=np.int64)
    i = np.arange(R, dtype=np.int64)
    valid = i[None, :] < r[:, None]
    with np.errstate(over="ignore"):
        ia = (i[:, None] * nc + np.arange(nc, dtype=np.int64)[None, :] + 1).astype(np.uint64)
        wa = _fin64(np.ascontiguousarray(A6, dtype=np.float64).view(np.uint64) + ia[None] * _HG)
        il = (r[:, None] * nc + i[None, :] + 1).astype(np.uint64)
        iu = (r[:, None] * nc + r[:, None] + i[None, :] + 1).astype(np.uint64)
        wl = _fin64(np.ascontiguousarray(L6, dtype=np.float64).view(np.uint64) + il * _HG)
        wu = _fin64(np.ascontiguousarray(U6, dtype=np.float64).view(np.uint64) + iu * _HG)
        zero = np.uint64(0)
        h = (np.where(valid[..., None], wa, zero).sum(axis=(1, 2), dtype=np.uint64) + np.where(valid, wl, zero).sum(axis=1, dtype=np.uint64)
             + np.where(valid, wu, zero).sum(axis=1, dtype=np.uint64))
        return _fin64(h ^ r.astype(np.uint64))


def finish_pieces_host(Ar, lr, ur, rows, flags, rec_of, ncols, take, xk, probe, n, m, member_tol=MEMBER_TOL, store_cap=None):
    """The numpy twin of Engine.finish_pieces (qpn_finish_pieces), for engines without it: _finish_host per record, then the
    status words, hashes, duplicates and the compacted store with the ABI's meaning (include/qpn_hip.h)."""
    Ar = np.asarray(Ar, dtype=np.float64); lr = np.asarray(lr, dtype=np.float64); ur = np.asarray(ur, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.int32); flags = np.asarray(flags, dtype=np.int32); rec_of = np.asarray(rec_of, dtype=np.int32)
    ncols = np.asarray(ncols, dtype=np.int32); take = np.asarray(take, dtype=np.int32)
    xk = np.asarray(xk, dtype=np.float64); probe = np.asarray(probe, dtype=np.float64)
    P, oc, cap = Ar.shape
    status = np.zeros(P, np.int32); worst = np.zeros(P); hsh = np.zeros(P, np.uint64); dup_of = np.full(P, -1, np.int32)
    status[flags != 0] = 8
    fin = {}
    for k in np.unique(rec_of[flags == 0]).tolist():
        plain = np.nonzero((rec_of == k) & (flags == 0))[0]
        nc = int(ncols[k])
        wk, A3, L2, U2, mg, A6, LU6 = _finish_host(Ar, lr, ur, rows, plain, take[k, :nc], xk[k, :nc], probe[k, :nc])
        hsh[plain] = _key_hash(A6, LU6[:, :cap], LU6[:, cap:], rows[plain])
        worst[plain] = wk
        status[plain] = np.where(wk <= member_tol, 1, 0) | np.where(mg, 2, 0)
        groups = {}
        for j, t in enumerate(plain.tolist()):
            fin[t] = (A3[j], L2[j], U2[j], nc)
            if status[t] != 1:
                continue
            r = int(rows[t])
            key = (A6[j, :r].tobytes(), LU6[j, :r].tobytes(), LU6[j, cap:cap + r].tobytes())
            for t2, key2 in groups.setdefault(int(hsh[t]), []):
                if key2 == key:
                    dup_of[t] = t2; status[t] |= 4
                    break
            else:
                groups[int(hsh[t])].append((t, key))
    src = [t for t in range(P) if (status[t] & 1) and not (status[t] & 12)]
    S = len(src)
    if store_cap is not None and S > store_cap:
        raise RuntimeError("finish_pieces: more pieces to store than store_cap")
    store_of = np.full(P, -1, np.int32)
    As = np.zeros((S, oc, cap)); ls = np.zeros((S, cap)); us = np.zeros((S, cap)); rows_s = np.zeros(S, np.int32)
    for q, t in enumerate(src):
        A3t, L2t, U2t, nc = fin[t]
        store_of[t] = q; As[q, :nc, :] = A3t.T; ls[q] = L2t; us[q] = U2t; rows_s[q] = rows[t]
    return dict(status=status, worst=worst, hash=hsh, dup_of=dup_of, store_of=store_of, As=As, ls=ls, us=us, rows_s=rows_s, stored=S)


# ---------------------------------------------------------------------------------------------------------------------
# multiplier-vertex exploration (QPNetOptions.exploration_vertices; src/avi_solutions.jl:92-129, :241-382)
# ---------------------------------------------------------------------------------------------------------------------
# Row classes of the multiplier set at the point, Lambda(x) = {lambda : Ad' lambda = g, per-row sign or zero}
MV_GE, MV_LE, MV_FREE, MV_ZERO = 0, 1, 2, 3
# status words of qpn_multiplier_vertices (include/qpn_hip.h)
MV_COMPLETE, MV_VERTEX_BUDGET, MV_BASIS_BUDGET, MV_EMPTY, MV_NO_VERTEX = 0, 1, 2, 3, 4
MV_TOL = 1e-9            # pivot and zero tolerance on the equilibrated rows
MV_FEAS = 1e-6           # a basic sign-constrained multiplier down to -MV_FEAS (times the rhs scale) counts as 0
MV_BAND = 1.0 - 2.0 ** -30
MV_BASES_PER_VERTEX = 64     # default basis budget: this many bases per vertex asked for


def multiplier_classes(m2):
    """The row classes of Lambda(x) from the GAVI codes of the constraint rows (comp_indices, refined): code 5 alone >= 0,
    code 7 alone <= 0, code 8 or both 5 and 7 free, code 6 alone = 0."""
    m2 = np.asarray(m2, dtype=np.uint8)
    b5 = (m2 >> 4) & 1 == 1; b7 = (m2 >> 6) & 1 == 1; b8 = (m2 >> 7) & 1 == 1
    cls = np.full(m2.shape, MV_ZERO, np.uint8)
    cls[b5 & ~b7] = MV_GE
    cls[b7 & ~b5] = MV_LE
    cls[b8 | (b5 & b7)] = MV_FREE
    return cls


def _mv_pivot(T, c, colof, tol):
    """One Gauss-Jordan step on column c over the rows not yet pivoted: the largest |entry|, entries within 2^-30 of it count as
    equal and the lowest row wins.  Returns the row, or -1 when every candidate is <= tol (the column depends on the pivoted ones)."""
    a = np.where(colof < 0, np.abs(T[:, c]), -1.0)
    amax = a.max() if a.size else -1.0
    if not amax > tol:
        return -1
    r = int(np.nonzero(a >= amax * MV_BAND)[0][0])
    p = T[r, c]
    T[r] = T[r] / p
    f = T[:, c].copy(); f[r] = 0.0
    T -= f[:, None] * T[r][None, :]
    colof[r] = c
    return r


def _mv_one(E, g, cls, lam0, V, max_bases, tol, feas):
    """multiplier_vertices_host for one item: (vertices [k, m], status)."""
    n, m = E.shape
    keep = cls != MV_ZERO
    sgn = cls == MV_GE
    sgn |= cls == MV_LE
    sig = np.where(cls == MV_LE, -1.0, 1.0)
    T0 = np.zeros((n, m + 1))
    T0[:, :m] = np.where(keep[None, :], E * sig[None, :], 0.0)
    T0[:, m] = g
    s = np.max(np.abs(T0[:, :m]), axis=1, initial=0.0)
    gs = max(1.0, float(np.max(np.abs(g), initial=0.0)))
    if np.any((s == 0.0) & (np.abs(g) > feas * gs)):
        return np.zeros((0, m)), MV_EMPTY
    nz = s > 0.0
    T0[nz] = T0[nz] / s[nz][:, None]
    T0[~nz, m] = 0.0
    gs = max(1.0, float(np.max(np.abs(T0[:, m]), initial=0.0)))
    free = np.nonzero(cls == MV_FREE)[0]
    mu = np.where(keep, sig * lam0, 0.0)
    mu = np.where(sgn & (mu < 0.0), 0.0, mu)
    # 1. purification: the support of mu is made independent by moving along null directions until a sign-constrained
    #    entry reaches 0 (the lowest such index when several do)
    while True:
        T = T0.copy(); colof = np.full(n, -1, np.int64); rowof = np.full(m, -1, np.int64)
        for c in free.tolist():
            r = _mv_pivot(T, c, colof, tol)
            if r < 0:
                return np.zeros((0, m)), MV_NO_VERTEX           # dependent free columns: Lambda(x) has a lineality space
            rowof[c] = r
        dep = -1
        for c in np.nonzero(sgn & (mu > tol))[0].tolist():
            r = _mv_pivot(T, c, colof, tol)
            if r < 0:
                dep = c
                break
            rowof[c] = r
        if dep < 0:
            break
        d = np.zeros(m); d[dep] = 1.0
        piv = np.nonzero(rowof >= 0)[0]
        d[piv] = -T[rowof[piv], dep]
        cand = sgn & ((rowof >= 0) | (np.arange(m) == dep))
        if np.any(cand & (d < -tol)):
            on = cand & (d < -tol); ratio = np.where(on, mu / np.where(on, -d, 1.0), np.inf); step = 1.0
        else:
            on = cand & (d > tol); ratio = np.where(on, mu / np.where(on, d, 1.0), np.inf); step = -1.0
        th = ratio.min()
        blk = int(np.nonzero(ratio <= th + th * 2.0 ** -30)[0][0])
        mu = mu + (step * th) * d
        mu[blk] = 0.0
        mu = np.where(sgn & (mu < 0.0), 0.0, mu)
    # 2. the rest of a basis, ascending; rows left without a pivot must have a zero right-hand side
    for c in np.nonzero(sgn & ~(mu > tol))[0].tolist():
        r = _mv_pivot(T, c, colof, tol)
        if r >= 0:
            rowof[c] = r
    if np.any((colof < 0) & (np.abs(T[:, m]) > feas * gs)):
        return np.zeros((0, m)), MV_EMPTY
    # 3. breadth-first walk over feasible bases (every basis factored afresh from T0, its columns in ascending order)
    visited = [frozenset(np.nonzero(rowof >= 0)[0].tolist())]
    seen = {visited[0]}
    overflow = False
    verts, keys = [], []
    head = 0
    status = MV_COMPLETE
    while head < len(visited):
        B = sorted(visited[head]); head += 1
        T = T0.copy(); colof = np.full(n, -1, np.int64); rowof = np.full(m, -1, np.int64)
        ok = True
        for c in B:
            r = _mv_pivot(T, c, colof, tol)
            if r < 0:
                ok = False
                break
            rowof[c] = r
        if not ok:
            continue
        mu = np.zeros(m)
        bas = np.array(B, dtype=np.int64)
        mu[bas] = T[rowof[bas], m]
        if np.any(sgn & (mu < -feas * gs)):
            continue
        mu = np.where(sgn & (mu < tol * gs), 0.0, mu)
        lam = sig * mu
        key = (np.round(lam, 5) + 0.0).tobytes()
        if key not in keys:
            if len(verts) == V:
                status = MV_VERTEX_BUDGET
                break
            keys.append(key); verts.append(lam)
        for j in range(m):
            if not sgn[j] or rowof[j] >= 0:
                continue
            th, rows = np.inf, []
            for c in B:
                if not sgn[c]:
                    continue
                a = T[rowof[c], j]
                if a > tol:
                    rt = mu[c] / a
                    rows.append((c, rt))
                    th = min(th, rt)
            if not rows:
                continue                                        # a ray: no vertex that way
            lim = th + th * 2.0 ** -30
            for c, rt in rows:
                if rt <= lim:
                    nb = visited[head - 1] - {c} | {j}
                    if nb in seen:
                        continue
                    if len(visited) >= max_bases:
                        overflow = True
                        continue
                    seen.add(nb); visited.append(nb)
    if status == MV_COMPLETE and overflow:
        status = MV_BASIS_BUDGET
    return (np.array(verts) if verts else np.zeros((0, m))), status


def multiplier_vertices_host(Ac, g, cls, lam0, V, max_bases=None, tol=MV_TOL, feas=MV_FEAS):
    """The numpy twin of Engine.multiplier_vertices (qpn_multiplier_vertices), for engines without it.  Per item: Ac [n, m]
    (the ABI layout of Ad, i.e. Ad'), g [n], the row classes cls [m] (MV_*), the multiplier lam0 [m] the vertex walk starts
    from; up to V vertices of Lambda(x) = {lambda : Ad' lambda = g, classes} in breadth-first order, distinct after rounding
    to 5 digits.  Returns (verts [batch, V, m], count [batch] int32, status [batch] int32)."""
    Ac = np.asarray(Ac, dtype=np.float64); g = np.asarray(g, dtype=np.float64)
    cls = np.asarray(cls, dtype=np.uint8); lam0 = np.asarray(lam0, dtype=np.float64)
    batch, n, m = Ac.shape
    max_bases = MV_BASES_PER_VERTEX * max(V, 1) if max_bases is None else int(max_bases)
    verts = np.zeros((batch, V, m)); count = np.zeros(batch, np.int32); status = np.zeros(batch, np.int32)
    for b in range(batch):
        vb, st = _mv_one(Ac[b], g[b], cls[b], lam0[b], V, max_bases, tol, feas)
        count[b] = len(vb); status[b] = st
        if len(vb):
            verts[b, :len(vb)] = vb
    return verts, count, status


def recipe_filter_host(masks, K, vrow_of, first_of):
    """The numpy twin of Engine.recipe_filter (qpn_recipe_filter): recipe t of virtual row v = vrow_of[t] is kept unless an
    earlier row s of the same item (first_of[v] <= s < v) holds it, i.e. every code of K[t] is in masks[s]: the reference's
    setdiff(Ks, explored_Ks) (src/avi_solutions.jl:129).  Returns keep [pieces] uint8."""
    masks = np.asarray(masks, dtype=np.uint8); K = np.asarray(K, dtype=np.uint8)
    vrow_of = np.asarray(vrow_of, dtype=np.int64); first_of = np.asarray(first_of, dtype=np.int64)
    keep = np.ones(K.shape[0], np.uint8)
    bit = (np.uint8(1) << (K.astype(np.uint8) - np.uint8(1))).astype(np.uint8)
    for t in range(K.shape[0]):
        v = int(vrow_of[t])
        for s in range(int(first_of[v]), v):
            if np.all(masks[s] & bit[t]):
                keep[t] = 0
                break
    return keep


def _box_count(masks):
    return float(np.prod([bin(int(v)).count("1") for v in masks]))


def distinct_recipes(prod_masks):
    """The number of distinct recipes over an item's products (boxes of codes), by inclusion-exclusion over earlier products."""
    total = 0.0
    for t in range(len(prod_masks)):
        earlier = list(range(t))
        for r in range(len(earlier) + 1):
            for S in itertools.combinations(earlier, r):
                mk = prod_masks[t].copy()
                for s in S:
                    mk &= prod_masks[s]
                total += (-1.0) ** r * _box_count(mk)
    return total


def _multiplier_vertices(eng, Ac, g, cls, lam0, V):
    fn = getattr(eng, "multiplier_vertices", None)
    if callable(fn):
        verts, count, status = fn(Ac, g, cls, lam0, V)
        return np.asarray(verts), np.asarray(count), np.asarray(status)
    return multiplier_vertices_host(Ac, g, cls, lam0, V)


def _recipe_filter(eng, masks, K, vrow_of, first_of):
    fn = getattr(eng, "recipe_filter", None)
    return fn(masks, K, vrow_of, first_of) if callable(fn) else recipe_filter_host(masks, K, vrow_of, first_of)


def explore_products(b, sel, rets, want, masks, total, tol, eng, E):
    """The recipe products of the wanted records of batch b with multiplier-vertex exploration (E = exploration_vertices >= 2):
    per item its own code sets, then the code sets (comp_indices at (x, v), refined as _piece_masks does) at up to E - 1
    vertices v of Lambda(x) that differ from the verified multiplier after rounding to 5 digits, in the breadth-first order of
    qpn_multiplier_vertices; a product whose code sets equal an earlier one of the item, or that has a row without a code, is
    left out.  One vertex call for the batch.  Returns dict(vsel, vmasks, vtotal, vfirst: one entry per product, grouped by
    item in the order of sel; distinct: per item the number of distinct recipes over its products)."""
    n, m = b.n, b.m
    xd, w = b.last["xd"], b.last["w"]
    sel_a = np.asarray(sel, dtype=np.int64)
    ok = total > 0
    extra = [[] for _ in sel]
    if m and ok.any():
        lam0 = np.zeros((len(sel), m))
        for t, k in enumerate(sel):
            lam0[t, :b.m_true[k]] = rets[b.where[k]]["lam"]
        g = np.einsum("bji,bj->bi", b.Qc[sel_a], xd[sel_a]) + np.einsum("bji,bj->bi", b.Rc[sel_a], w[sel_a]) + b.qd[sel_a]
        cls = multiplier_classes(masks[:, n:])
        on = np.nonzero(ok & np.any(cls != MV_ZERO, axis=1))[0]
        if on.size:
            verts, count, status = _multiplier_vertices(eng, b.Ac[sel_a[on]], g[on], cls[on], lam0[on], E)
            vk, vl = [], []
            for q, t in enumerate(on.tolist()):
                key0 = (np.round(lam0[t], 5) + 0.0).tobytes()
                got = 0
                for j in range(int(count[q])):
                    v = verts[q, j]
                    if (np.round(v, 5) + 0.0).tobytes() == key0:
                        continue
                    if got == E - 1:
                        break
                    vk.append(t); vl.append(v); got += 1
            if vk:
                vk = np.asarray(vk)
                rows = sel_a[vk]
                lam = np.asarray(vl)
                r1 = np.einsum("bji,bj->bi", b.Qc[rows], xd[rows]) + np.einsum("bji,bj->bi", b.Rc[rows], w[rows]) + b.qd[rows] \
                    - np.einsum("bij,bj->bi", b.Ac[rows], lam)
                s = np.einsum("bji,bj->bi", b.Ac[rows], xd[rows]) + np.einsum("bji,bj->bi", b.Bc[rows], w[rows])
                free_lo = np.full((rows.size, n), -INF); free_hi = np.full((rows.size, n), INF)
                m1 = np.asarray(eng.comp_indices(xd[rows], r1, free_lo, free_hi, tol=tol, shift=0))
                m2 = np.asarray(eng.comp_indices(s, lam, b.l[rows], b.u[rows], tol=tol, shift=4))
                for q, k in enumerate(rows.tolist()):
                    m2[q, b.m_true[k]:] = 1 << 5
                m2 = _refine_row_codes(m2, s, lam, b.l[rows], b.u[rows], CODE_TOL)
                vm = np.concatenate([m1, m2], axis=1).astype(np.uint8)
                for q, t in enumerate(vk.tolist()):
                    if not np.any(vm[q] == 0):
                        extra[t].append(vm[q])
    vsel, vmasks, vfirst, distinct = [], [], [], np.zeros(len(sel))
    for t, k in enumerate(sel):
        prods = [masks[t]] if ok[t] else []
        for mk in extra[t]:
            if not any(np.array_equal(mk, p_) for p_ in prods):
                prods.append(mk)
        f0 = len(vsel)
        for p_ in prods:
            vsel.append(k); vmasks.append(p_); vfirst.append(f0)
        distinct[t] = distinct_recipes(prods) if prods else 0.0
    N = masks.shape[1]
    vmasks = np.asarray(vmasks, dtype=np.uint8).reshape(len(vsel), N)
    vtotal = np.array([_box_count(mk) for mk in vmasks], dtype=np.float64)
    return dict(vsel=np.asarray(vsel, dtype=np.int64), vmasks=vmasks, vtotal=vtotal, vfirst=np.asarray(vfirst, dtype=np.int32),
                distinct=distinct)


def _recipe_rounds(eng, vm, vt, vf, cap, chunk, filtered, up, down):
    """The one source of recipes.  A row is a product of codes (vm [rows, N], vt [rows] its recipes); an item's rows are
    consecutive and share vf, the item's first row.  The rule: an item keeps its products in order, each in its own recipe
    order, minus -- when `filtered` -- the recipes an earlier product of the item holds (recipe_filter), cut after `cap`
    recipes (None: not cut).  Yields rounds (K, row_of) with the rows ascending; an item's recipes keep that order over the rounds.
    How the windows lie is efficiency, not meaning.  With a cap: one window per item and pass, on the item's first live
    unspent row and no longer than what the item still needs, pass after pass until every item is full or spent; the passes
    make ONE round.  Without a filter that is one pass whose windows all start at recipe 0: the plain recipes_batch call.  Every
    other layout is ranged, its first round included, and asks once whether the engine takes `first`: the entries called and
    their number stay what they were when each layout had a body of its own.  cap None: consecutive rows until a round holds
    `chunk` recipes.
    (up, down): the arrays' home, see solution_pieces; the masks go there once."""
    rows = vm.shape[0]
    # (a product of 64 two-code rows has 2^64 recipes: the float counts are bounded before the cast; no window runs past the
    #  cap, or past MAX_RECIPES without one)
    vt = np.minimum(vt, 2.0 ** 62).astype(np.int64)
    live = vt > 0
    vm_h = up(vm)
    if filtered:
        # a product that holds no recipe of its own (every one lies in an earlier product of the item) is skipped outright
        for v in np.nonzero(live & (np.arange(rows) > vf))[0].tolist():
            live[v] = distinct_recipes(list(vm[vf[v]:v + 1])) > distinct_recipes(list(vm[vf[v]:v]))
        vf_h = up(vf)
    plain = cap is not None and not filtered
    ranged = None                                        # does recipes_batch take `first`?  Asked off the plain path only

    def window(act, first, cnt):
        nonlocal ranged
        offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        if plain:
            K, _ = eng.recipes_batch(vm[act], offsets)
        else:
            if ranged is None:
                ranged = _supports_first(eng)
            K, _ = eng.recipes_batch(vm_h[up(act)], offsets, first=first) if ranged else _recipes_range_host(vm[act], first, cnt)
        row_of = np.repeat(act, cnt)
        if filtered:
            keep = _recipe_filter(eng, vm_h, K, up(row_of.astype(np.int32)), vf_h) != 0
            K, row_of = K[keep], row_of[down(keep)]
        return K, row_of

    if cap is None:
        lv = np.nonzero(live)[0]
        G = np.concatenate([[0], np.cumsum(vt[lv])]).astype(np.int64)
        for c0 in range(0, int(G[-1]), chunk):
            lo = np.maximum(G[:-1], c0); hi = np.minimum(G[1:], c0 + chunk)
            part = np.nonzero(hi > lo)[0]                # the rows with recipes in this round
            K, row_of = window(lv[part], lo[part] - G[:-1][part], hi[part] - lo[part])
            if row_of.size:
                yield K, row_of
        return
    cur = np.zeros(rows, np.int64)                       # per row: the next recipe to enumerate
    got = np.zeros(rows, np.int64)                       # per item (at its first row): recipes kept so far
    Ks, rs = [], []
    while True:
        act = np.nonzero(live & (cur < vt) & (got[vf] < cap))[0]
        act = act[np.unique(vf[act], return_index=True)[1]]                         # the first such row of every item
        if not act.size:
            break
        need = cap - got[vf[act]]
        cnt = np.minimum(vt[act] - cur[act], need)
        K, row_of = window(act, cur[act], cnt)
        got[vf[act]] += np.bincount(row_of, minlength=rows)[act]                    # (the filter may have left fewer than cnt)
        cur[act] += cnt
        Ks.append(np.asarray(K)); rs.append(row_of)
    if len(rs) > 1:
        order = np.argsort(np.concatenate(rs), kind="stable")
        Ks, rs = [np.concatenate(Ks)[order]], [np.concatenate(rs)[order]]
    if rs:
        yield Ks[0], rs[0]


def _recipes_range_host(masks, first, counts):
    """qpn_recipes_batch_range restated (engines whose recipes_batch has no `first`): node b's recipes first[b] .. first[b] +
    counts[b] - 1 of its Cartesian product, row 0 the fastest digit."""
    masks = np.asarray(masks, dtype=np.uint8)
    nodes, N = masks.shape
    K = np.zeros((int(np.sum(counts)), N), np.uint8); node_of = np.repeat(np.arange(nodes, dtype=np.int32), counts)
    o = 0
    for b in range(nodes):
        cnt = int(counts[b])
        idx = int(first[b]) + np.arange(cnt, dtype=np.int64)
        for i in range(N):
            codes = np.array([c + 1 for c in range(8) if (int(masks[b, i]) >> c) & 1], dtype=np.uint8)
            if codes.size:
                K[o:o + cnt, i] = codes[idx % codes.size]; idx = idx // codes.size
        o += cnt
    return K, node_of


def _record_spans(rec_of):
    """(record, first piece, end) for a round whose pieces come record by record, ascending."""
    ks, starts = np.unique(rec_of, return_index=True)
    return zip(ks.tolist(), starts.tolist(), starts.tolist()[1:] + [len(rec_of)])


def _read_lean(eng, b, K, rec_of, colsel, x, member_tol, projected):
    """A round read on the host, the capped route's reader: reduced_pieces, then _finish_host record by record -- no hashes, no
    store, and one record's finished rows alive at a time.  Yields per record (k, first piece t0, status and worst of its
    pieces as lists, piece, spare).  Status as qpn_finish_pieces writes it: 1 member, 2 merge candidate, 8 flagged.  piece(t)
    -> the finished rows (A, l, u) of plain piece t and its key in the node's piece set, None for a merge candidate;
    spare(t) -> a non-member's rows held for the node's fallback: a call gives (A, l, u).
    (The status, worst and row counts are Python lists and the records come one by one on purpose: the default path has about
    one piece per record, so its cost is what is done per record, and a record's rows are megabytes at n = m = 32.)"""
    from .avi_solutions import _probe_vector
    recd, K = (b.Qc, b.Rc, b.qd, b.Ac, b.Bc, b.l, b.u), np.asarray(K)
    Ar, lr, ur, rows, flags = (np.asarray(a) for a in eng.reduced_pieces(*recd, K, rec_of))
    projected.update(_project_flagged(eng, recd, K, rec_of, flags, b.n, b.m))
    Rmax, rows_l = Ar.shape[2], rows.tolist()
    for k, t0, t1 in _record_spans(rec_of):
        cols_k, take_k = colsel[k]
        st, worst, at = [8] * (t1 - t0), [0.0] * (t1 - t0), {}
        plain = t0 + np.nonzero(flags[t0:t1] == 0)[0]
        if plain.size:
            wk, A3, L2, U2, merge, A6, LU6 = _finish_host(Ar, lr, ur, rows, plain, take_k, x[cols_k], _probe_vector(len(cols_k)))
            # the parent's verify_solution tests feasibility on exactly these normalised rows with 1e-3 (src/qp_processing.jl:86):
            # a piece the point fails here would be "infeasible" there by construction (MEMBER_TOL)
            merge = merge.tolist()
            for j, (t, w, mg) in enumerate(zip(plain.tolist(), wk.tolist(), merge)):
                st[t - t0], worst[t - t0], at[t] = (w <= member_tol) + 2 * mg, w, j
        ckey = cols_k.tobytes()

        def piece(t):
            j, r = at[t], rows_l[t]
            key = None if merge[j] else (ckey, A6[j, :r].tobytes(), np.concatenate([LU6[j, :r], LU6[j, Rmax:Rmax + r]]).tobytes())
            return A3[j, :r].copy(), L2[j, :r].copy(), U2[j, :r].copy(), key

        def spare(t):
            held = piece(t)[:3]                          # (copies: the record's arrays go when the next record is read)
            return lambda: held
        yield k, t0, st, worst, piece, spare


def _read_store(eng, finish, b, recd, fin_in, K, rec_of, colsel, x, member_tol, up, down, projected):
    """A round read through the ABI's store, the uncapped route's reader: reduced_pieces, then `finish` where the arrays live
    (the engine's finish_pieces on the device, whence only the store and the per-piece words come back; finish_pieces_host,
    the kernel's twin, on the host).  Status bit 4: a member equal to an earlier one of the round.  Yields what _read_lean
    yields; a non-member is not in the store: spare keeps its reduced rows, and _finish_host finishes them, bit-equal to the
    device, only if the node still needs them in the end."""
    from .avi_solutions import _probe_vector
    rec_h = up(rec_of)
    red = eng.reduced_pieces(*recd, K, rec_h)
    fin = finish(*red, rec_h, *fin_in, b.n, b.m, member_tol=member_tol)
    st, worst, store_of, As, ls, us, rows_s = (down(fin[key]) for key in ("status", "worst", "store_of", "As", "ls", "us", "rows_s"))
    projected.update(_project_flagged(eng, recd, K, rec_h, st & 8, b.n, b.m, down))       # (status bit 8: flagged)
    rec_l, store_of, rows_s, merged = rec_of.tolist(), store_of.tolist(), rows_s.tolist(), (st & 2).tolist()

    def piece(t):
        cols_k, j = colsel[rec_l[t]][0], store_of[t]
        r = rows_s[j]
        A, l, u = np.ascontiguousarray(As[j, :len(cols_k), :r].T), ls[j, :r].copy(), us[j, :r].copy()
        key = None if merged[t] else (cols_k.tobytes(), (np.round(A, 6) + 0.0).tobytes(), np.round(np.concatenate([l, u]), 6).tobytes())
        return A, l, u, key

    def spare(t):
        one = [down(a[t:t + 1]) for a in red[:4]]        # the reduced rows are kept, and finished only if the node needs them in the end
        cols_k, take_k = colsel[rec_l[t]]

        def rows():
            _, A3, L2, U2, _, _, _ = _finish_host(*one, np.zeros(1, np.int64), take_k, x[cols_k], _probe_vector(len(cols_k)))
            r = int(one[3][0])
            return A3[0, :r].copy(), L2[0, :r].copy(), U2[0, :r].copy()
        return rows
    st, worst = st.tolist(), worst.tolist()
    for k, t0, t1 in _record_spans(rec_of):
        yield k, t0, st[t0:t1], worst[t0:t1], piece, spare


def solution_pieces(qpn, recs, batches, rets, x, engine, want: Sequence[bool], tol=1e-2, max_pieces=64, member_tol=MEMBER_TOL,
                    truncated=None, _chunk=None, exploration_vertices=0):
    """The solution-graph pieces of MANY nodes around (x, lambda) (process_solution_graph, src/avi.jl:447-477 ->
    comp_indices -> all_Ks, src/avi_solutions.jl:200-215 -> local_piece, :400-496 -> the multipliers eliminated, the
    columns permuted back, :86-87), batched: per record shape one comp_indices pair, one recipes call, one pieces call.
    Returns a list (per item; None where `want` is False) of lists of Poly in global coordinates.
    max_pieces: the first that many recipes of each item (a UserWarning names an item that has more; its index goes into the
    set `truncated` when one is given); None: every recipe, chunk by chunk (_chunk overrides the chunk size), finished on the
    device when the engine has finish_pieces (its numpy twin otherwise).
    exploration_vertices E >= 2: the recipes of up to E - 1 further vertices of the multiplier set Lambda(x) join each item's
    own (explore_products); a recipe an earlier product of the item holds is skipped, and max_pieces counts the distinct
    recipes of the item.  E <= 1 launches nothing new.

    One pipeline serves every mode: _recipe_rounds is the source of recipes, a round is read by _read_lean (a cap) or
    _read_store (None), and its pieces are admitted below, in recipe order.  The modes differ in the windows' layout and in the
    reader, nowhere else.  The pieces of a round that the device elimination flags (degenerate active sets) are projected in one
    project_pieces call by the round's reader when the engine has that method (_project_flagged), piece by piece on the host
    otherwise (_reduce_on_host); the pieces are the same either way."""
    from .avi_solutions import _dedupe, _probe_vector
    eng = engine
    x = np.asarray(x, dtype=np.float64)
    out: List[Optional[list]] = [None] * len(recs)
    # the arrays' home, chosen once: the device for the uncapped route of an engine that finishes pieces there, else the host
    if max_pieces is None and callable(getattr(eng, "finish_pieces", None)) and getattr(eng, "device", -1) >= 0:
        import torch
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=f"cuda:{eng.device}")
        down = lambda a: a.cpu().numpy()
        finish = eng.finish_pieces
    else:
        up, down, finish = (lambda a: a), np.asarray, finish_pieces_host

    def build(cols_k, A, l, u, merge):
        Pg = Poly.from_sorted(qpn.num_vars, cols_k, A, l, u, normalise=False)
        return _dedupe(Pg) if merge else Pg
    for b in batches:
        sel = [k for k, i in enumerate(b.where) if want[i]]
        if not sel:
            continue
        n, m, p = b.n, b.m, b.p
        masks, total = _piece_masks(b, sel, rets, want, tol, eng)
        # the rows: one per wanted record, or the products of its explored vertices
        vsel, vm, vt, vf, distinct = np.asarray(sel), masks, total, np.arange(len(sel), dtype=np.int32), total
        if exploration_vertices >= 2:
            ex = explore_products(b, sel, rets, want, masks, total, tol, eng, exploration_vertices)
            vsel, vm, vt, vf, distinct = ex["vsel"], ex["vmasks"], ex["vtotal"], ex["vfirst"], ex["distinct"]
        for t in np.nonzero(distinct > (MAX_RECIPES if max_pieces is None else max_pieces))[0].tolist():
            pid = recs[b.where[sel[t]]]["pid"]
            if max_pieces is None:
                raise RuntimeError(f"node {pid}: {int(distinct[t])} local recipes, more than the 2^24 the uncapped solution graph "
                                   "(max_pieces=None) enumerates")
            warnings.warn(f"node {pid}: {int(distinct[t])} local recipes, only the first {max_pieces} are expanded (max_pieces)")
            if truncated is not None:
                truncated.add(b.where[sel[t]])
        for k in sel:
            out[b.where[k]] = []                         # (an item without a recipe keeps an empty graph)
        colsel = {k: _colsel(b, k) for k in sel}         # per record: the piece's columns [x_d; x_p present] in ascending order
        chunk = _chunk
        if max_pieces is None:
            oc, cap, N = n + p, n + 2 * m, n + m
            if chunk is None:
                # per piece: K, reduced_pieces' output and its local-piece workspace, finish_pieces' scratch and store
                chunk = max(1, CHUNK_BYTES // (N + 8 * (2 * (oc * cap + 2 * cap + 1) + 2 * N * (N + p) + 4 * N + 4 * cap + 4) + 64))
            take = np.zeros((len(b), oc), np.int32); ncols = np.zeros(len(b), np.int32); xk = np.zeros((len(b), oc)); probe = np.zeros((len(b), oc))
            for k, (cols_k, take_k) in colsel.items():
                nc = len(cols_k)
                ncols[k] = nc; take[k, :nc] = take_k; xk[k, :nc] = x[cols_k]; probe[k, :nc] = _probe_vector(nc)
            recd = tuple(up(a) for a in (b.Qc, b.Rc, b.qd, b.Ac, b.Bc, b.l, b.u))  # (on the device: the records go up once per batch)
            fin_in = tuple(up(a) for a in (ncols, take, xk, probe))
        seen = {b.where[k]: set() for k in sel}          # per node: the keys of its pieces (the reference collects them in a
                                                         # Set, src/avi_solutions.jl:104)
        fallback = {}                                    # per node: (miss, Poly or (columns, spare rows, merge)) of the piece the point misses
                                                         # least, first on ties, for a node none of whose pieces passes (a solution
                                                         # graph is never empty, src/qp_processing.jl:233)
        for K, row_of in _recipe_rounds(eng, vm, vt, vf, max_pieces, chunk, exploration_vertices >= 2, up, down):
            rec_of = vsel[row_of].astype(np.int32)       # recipe -> record inside the batch (records ascend)
            projected = {}                               # flagged piece -> its projected rows: filled by the reader, in one call
                                                         # per round, before it yields the first record
            if max_pieces is None:
                records = _read_store(eng, finish, b, recd, fin_in, K, rec_of, colsel, x, member_tol, up, down, projected)
            else:
                records = _read_lean(eng, b, K, rec_of, colsel, x, member_tol, projected)
            for k, t0, st, worst, piece, spare in records:
                i = b.where[k]
                cols_k, take_k = colsel[k]
                seen_i, out_i = seen[i], out[i]
                for t, (s_, miss) in enumerate(zip(st, worst), t0):     # (the miss is the finished rows', taken before _dedupe)
                    if s_ & 4:                           # an equal earlier piece of this round is in the set already
                        continue
                    if s_ & 8:                           # flagged by the device elimination: its projected rows, or the host restatement
                        raw = projected.get(t)
                        Pg, miss = _flagged_piece(qpn, b, k, down(K[t]) if raw is None else None, eng, cols_k, take_k, x, raw)
                        if Pg is None:
                            continue
                        member, key = miss <= member_tol, None
                    else:
                        member, Pg = s_ & 1, None
                    if not member:                       # kept only while it is the node's fallback, and not built before the end
                        if not out_i and (i not in fallback or miss < fallback[i][0]):
                            fallback[i] = (miss, Pg if s_ & 8 else (cols_k, spare(t), s_ & 2))
                        continue
                    if Pg is None:
                        A, l, u, key = piece(t)
                        if key is None:                  # a merge candidate: keyed, as a flagged piece, by what _dedupe leaves
                            Pg = build(cols_k, A, l, u, True)
                    if key is None:
                        key = _poly_key(Pg)
                    if key not in seen_i:
                        seen_i.add(key)
                        out_i.append(Poly.from_sorted(qpn.num_vars, cols_k, A, l, u, normalise=False) if Pg is None else Pg)
        for i, (miss, Pg) in fallback.items():
            if not out[i]:
                out[i].append(Pg if isinstance(Pg, Poly) else build(Pg[0], *Pg[1](), Pg[2]))
    return out


# rows of room per piece in the batched projection of a round's flagged pieces (Engine.project_pieces): PROJECT_CAP_FACTOR times
# the n + 2m rows a piece starts with, inside [PROJECT_CAP_MIN, PROJECT_CAP_MAX].  Any value keeps the results: a piece that needs
# more comes back with flag 4 and takes the per-piece route (_reduce_on_host), whose own limit is PROJECT_CAP_MAX rows.
PROJECT_CAP_MIN, PROJECT_CAP_FACTOR, PROJECT_CAP_MAX = 256, 4, 4096


def project_cap(n, m):
    return max(n + 2 * m, min(PROJECT_CAP_MAX, max(PROJECT_CAP_MIN, PROJECT_CAP_FACTOR * (n + 2 * m))))


def project_pieces_host(Ap, lp, up, keep, n, m, tol=1e-9, cap=None):
    """The numpy twin of qpn_project_pieces from the lifted pieces on (local_pieces' output: Ap [pieces, N+p, 2N] column-major
    per piece, lp, up, keep [pieces, 2N]): the multipliers eliminated through each piece's equality rows, then one
    Fourier-Motzkin step per column that no equality pins (avi_solutions.project_rows, the entry's arithmetic contract).
    Returns (Ar [pieces, n+p, cap] column-major per piece, lr, ur [pieces, cap], rows, flags [pieces]) with the entry's fill
    (0, -inf, +inf beyond rows[t]) and flags: 2 = more than cap rows alive after the equalities (the first cap go out, no
    Fourier-Motzkin step), 4 = a step needed more than cap rows (all fill, rows 0).  cap >= n + 2m; default project_cap(n, m)."""
    from .avi_solutions import fourier_motzkin, pin_multipliers
    Ap, lp, up, keep = np.asarray(Ap, dtype=np.float64), np.asarray(lp, dtype=np.float64), np.asarray(up, dtype=np.float64), np.asarray(keep)
    n, m = int(n), int(m)
    cap = project_cap(n, m) if cap is None else int(cap)
    if cap < n + 2 * m:
        raise ValueError("project_pieces_host: cap < n + 2m")
    pieces, cols = Ap.shape[0], Ap.shape[1]
    ycols = [c for c in range(cols) if c < n or c >= n + m]
    Ar = np.zeros((pieces, len(ycols), cap)); lr = np.full((pieces, cap), -INF); ur = np.full((pieces, cap), INF)
    rows = np.zeros(pieces, np.int32); flags = np.zeros(pieces, np.int32)
    for t in range(pieces):
        kept = keep[t].astype(bool)
        A, l, u, left = pin_multipliers(Ap[t].T[kept], lp[t][kept], up[t][kept], n, m, tol)
        if A.shape[0] > cap:
            flags[t] = 2
            A, l, u = A[:cap], l[:cap], u[:cap]
        else:
            out = fourier_motzkin(A, l, u, left, tol, cap)
            if out is None:
                flags[t] = 4
                continue
            A, l, u = out
        r = A.shape[0]
        Ar[t, :, :r] = A[:, ycols].T; lr[t, :r] = l; ur[t, :r] = u; rows[t] = r
    return Ar, lr, ur, rows, flags


def _poly_key(Pg):
    """The key of a piece in its node's piece set: columns, rows rounded to 6 digits (no negative zeros), bounds rounded."""
    cl, Al_ = Pg.local()
    return (cl.tobytes(), (np.round(Al_, 6) + 0.0).tobytes(), np.round(np.concatenate([Pg.l, Pg.u]), 6).tobytes())


def _project_flagged(eng, recd, K, rec_of, flags, n, m, down=np.asarray):
    """The flagged pieces of a round through the engine's project_pieces, ALL IN ONE CALL (qpn_project_pieces: the equality
    elimination again and the Fourier-Motzkin steps, on the device).  recd, K, rec_of: what the round's reduced_pieces call took
    (host arrays or device tensors); flags: nonzero for its flagged pieces, on the host.  -> {piece: the raw rows (A, l, u) over [x_d; x_p]}; a piece that does not
    fit project_cap rows is left out and takes the per-piece route.  {} for an engine without the method."""
    project = getattr(eng, "project_pieces", None)
    if not callable(project):
        return {}
    idx = np.nonzero(flags)[0]
    if not idx.size:
        return {}
    sel = idx
    if not isinstance(K, np.ndarray):
        import torch
        sel = torch.as_tensor(idx, device=K.device)
    Ar, lr, ur, rows, fl = (down(a) for a in project(*recd, K[sel], rec_of[sel], cap=project_cap(n, m)))
    return {t: (np.ascontiguousarray(Ar[i, :, :rows[i]].T), lr[i, :rows[i]].copy(), ur[i, :rows[i]].copy())
            for i, t in enumerate(idx.tolist()) if fl[i] == 0}


def _flagged_piece(qpn, b, k, Krow, eng, cols_k, take_k, x, raw=None):
    """A piece the device elimination flagged, normalised and merged; (Poly, miss) or (None, None).  raw: its projected rows from
    the round's project_pieces call (_project_flagged); without them, the host restatement piece by piece."""
    from .avi_solutions import _dedupe
    P = Poly(*raw).vectorize() if raw is not None else _reduce_on_host(b, k, Krow, eng)
    if P is None:
        return None, None
    Ah = np.ascontiguousarray(P[0][:, take_k]); big = np.max(np.abs(Ah), axis=1, initial=0.0)
    sc = np.where(big > 0.0, 1.0 / np.where(big > 0.0, big, 1.0), 1.0)
    with np.errstate(invalid="ignore"):
        Pg = _dedupe(Poly.from_sorted(qpn.num_vars, cols_k, Ah * sc[:, None], P[1] * sc, P[2] * sc))
    cl, Al_ = Pg.local()
    axp = Al_ @ x[cl]
    return Pg, float(np.max(np.maximum(Pg.l - axp, axp - Pg.u), initial=0.0))


def _supports_first(eng):
    import inspect
    try:
        return "first" in inspect.signature(eng.recipes_batch).parameters
    except (TypeError, ValueError):
        return False


def _refine_row_codes(m2, s, lam, l, u, mt):
    """Of the codes comp_indices allows on a constraint row (tolerance 1e-2), keep those whose OWN condition the point meets
    within `mt`: code 5 (s = l, lambda >= 0), 6 (lambda = 0, l <= s <= u), 7 (s = u, lambda <= 0), 8 (l = s = u).  A recipe's piece
    contains the point exactly when every row's condition holds (the lifted piece is a product of per-row conditions, src/
    avi_solutions.jl:413-432), so after this every enumerated recipe's piece contains the point -- see MEMBER_TOL.  A row left
    without any code keeps the allowed code it violates least."""
    viol = np.full(m2.shape + (4,), np.inf)
    with np.errstate(invalid="ignore"):
        viol[..., 0] = np.maximum(np.abs(s - l), np.maximum(-lam, 0.0))
        viol[..., 1] = np.maximum(np.abs(lam), np.maximum(np.maximum(l - s, s - u), 0.0))
        viol[..., 2] = np.maximum(np.abs(s - u), np.maximum(lam, 0.0))
        viol[..., 3] = np.maximum(np.abs(s - l), np.abs(s - u))
    viol = np.where(np.isnan(viol), np.inf, viol)
    bits = (m2[..., None] >> np.arange(4, 8)) & 1
    viol = np.where(bits == 1, viol, np.inf)
    keep = viol <= mt
    best = np.argmin(viol, axis=-1)
    none = ~keep.any(axis=-1) & (m2 != 0)
    keep[none, best[none]] = True
    out = np.zeros_like(m2)
    for c in range(4):
        out |= (keep[..., c].astype(np.uint8) << (4 + c)).astype(np.uint8)
    return out


def _reduce_on_host(b, k, Krow, eng):
    """A piece the device elimination flagged (a multiplier no equality row pins: Fourier-Motzkin, polyhedral) goes
    through the host restatement (avi_solutions.eliminate_multipliers)."""
    from .avi_solutions import eliminate_multipliers
    Ap, lp, up, keep = eng.local_pieces(b.Qc[k:k + 1], b.Rc[k:k + 1], b.qd[k:k + 1], b.Ac[k:k + 1], b.Bc[k:k + 1], b.l[k:k + 1],
                                        b.u[k:k + 1], np.asarray(Krow, dtype=np.uint8)[None], node_of=np.zeros(1, np.int32))
    rows = np.asarray(keep[0]).astype(bool)
    P = Poly(np.asarray(Ap[0]).T[rows], np.asarray(lp[0])[rows], np.asarray(up[0])[rows], normalise=False)
    try:
        Pl = eliminate_multipliers(P, b.n, b.m)
    except RuntimeError:
        return None
    return Pl.vectorize()


def process_level(qpn, players: Sequence[int], x, S: Dict[int, list], engine=None, exploration_vertices=0):
    """results = map(process_qp(qpn, id, x, S) for id in players) (src/algorithm.jl:44-52) as batches: every node under
    every combination of its children's pieces (src/qp_processing.jl:162-205) in one verify call per record shape, the
    solution graphs of the optimal ones in one call chain per record shape.  Returns one process_qp result per player."""
    from .avi import _eng
    from .qp_processing import combine_many
    eng = _eng(engine)
    x = np.asarray(x, dtype=np.float64)
    # process_qp is a function of x on the node's subtree columns and of its children's solution graphs: a node for which
    # neither has changed since the last sweep gets the result it got then (the reference recomputes it, src/algorithm.jl:47 --
    # to the same value).  On a net of many independent clusters most nodes are at rest after the first sweeps.
    memo = qpn.__dict__.setdefault("_process_memo", {})
    all_players = list(players)
    xkey = {pid: x[_subtree_cols(qpn, pid)].tobytes() for pid in all_players}
    hits = {}
    for pid in all_players:
        ent = memo.get(pid)
        if ent is not None and ent["xkey"] == xkey[pid] and ent["ev"] == exploration_vertices and \
                all(S.get(j) is g for j, g in ent["kids"].items()):
            hits[pid] = ent["result"]
    all_leaf_level = all(not qpn.network_edges[pid] for pid in all_players)
    if not all_leaf_level:
        players = [pid for pid in all_players if pid not in hits]      # (a level of childless nodes keeps its one resident batch:
                                                                       #  all are verified in one launch, hits skip the pieces)
    items, owner = [], []
    combos_of = {}
    for pid in players:
        children = sorted(qpn.network_edges[pid])
        if children:
            cards = [range(len(S[j])) for j in children]
            if any(len(c) < 1 for c in cards):
                raise RuntimeError("Solution graphs were not properly populated.")
            combos = list(itertools.product(*cards))
        else:
            combos = [()]
        combos_of[pid] = (children, combos)
        for combo in combos:
            items.append((pid, [S[j][ji] for j, ji in zip(children, combo)]))
            owner.append(pid)
    # (SUBSET_VERIFY_ROUTE: on an all-leaf level item i is player i; the hits' items are not verified again)
    only = None
    if SUBSET_VERIFY_ROUTE and all_leaf_level and hits:
        only = [i for i, pid in enumerate(owner) if pid not in hits]
    recs, batches, rets = verify_items(qpn, items, x, eng, check_convexity=qpn.options.check_convexity, only=only)
    results = dict(hits)                                                            # (a hit's result is the memo's)
    first = {}
    for i, (pid, _) in enumerate(items):
        first.setdefault(pid, i)
    want = [False] * len(items)
    for pid in players:
        children, combos = combos_of[pid]
        i0 = first[pid]
        if pid in hits:
            continue
        fail = next((t for t in range(len(combos)) if not rets[i0 + t]["solution"]), None)
        if fail is not None:                                                        # the first failure in product order, :206-216
            results[pid] = dict(solution=False, e=rets[i0 + fail]["e"], failed=False,
                                subpiece_assignments={j: ji for j, ji in zip(children, combos[fail])} if children else {})
            continue
        gen = (pid not in qpn.network_depth_map[1]) or qpn.options.gen_solution_map
        results[pid] = dict(solution=True, S=None, failed=False, truncated=False)
        if gen:
            for t in range(len(combos)):
                want[i0 + t] = True
    if any(want):
        cut = set()                                                                 # items whose graph the cap cut short
        pieces = solution_pieces(qpn, recs, batches, rets, x, eng, want, max_pieces=qpn.options.max_pieces, truncated=cut,
                                 exploration_vertices=exploration_vertices)
        jobs, job_pid = [], []
        for pid in players:
            children, combos = combos_of[pid]
            i0 = first[pid]
            if not want[i0]:
                continue
            per_combo = [pieces[i0 + t] for t in range(len(combos))]
            results[pid]["truncated"] = any(i0 + t in cut for t in range(len(combos)))
            if len(combos) == 1:
                results[pid]["S"] = per_combo[0]                                    # combine(...) with one solution set, :271-272
            else:
                jobs.append(([[S[j][ji] for j, ji in zip(children, combo)] for combo in combos], per_combo))
                job_pid.append(pid)
        if jobs:                                                                    # all kinks of the level: one batch of LPs,
            for pid, got in zip(job_pid, combine_many(jobs, x, eng, route=None)):   # on qp_processing.EMPTINESS_ROUTE
                if isinstance(got, RuntimeError):
                    results[pid] = dict(solution=False, failed=True, S=None)        # :219-223
                else:
                    results[pid]["S"] = got
        for pid in players:
            if results[pid].get("solution") and want[first[pid]] and len(results[pid]["S"]) == 0:
                raise RuntimeError("This shouldn't happen. Solution graph is empty.")
    for pid in all_players:
        if pid not in hits:
            memo[pid] = dict(xkey=xkey[pid], ev=exploration_vertices, result=results[pid],
                             kids={j: S.get(j) for j in qpn.network_edges[pid]})
    return [results[pid] for pid in all_players]
