"""Which KIND of iteration follows which in the Stage B pivot loop (the Lemke loop of csrc/qpn_avi_schur.hip), for the state
that the loop carries from one iteration into the next -- the entering column c, the entering variable's own travel limit
self_lim, the bounds elo / ehi it will have as a basic variable, the direction sigma and the pivot count.  A kernel that keeps
that state in scalar registers across the loop's joins is wrong exactly when one kind of iteration leaves a value that the
next kind reads, so the unit of coverage here is the ordered PAIR of kinds, not the kind.

`labelled_walk` is the walk of tests/stage_b_lemke.py (same rules, same arithmetic) that names every iteration:

  first             the first pivot: the artificial variable enters from the extra (covering) column, a p_k leaves
  p_lo, p_hi        a basis change in which p_k leaves at its lower / upper bound (d_k enters next, unlimited)
  d_two, d_one      a basis change in which the multiplier d_k leaves at 0, of a pair bounded on both sides / on one side only
                    (p_k enters next; its travel limit is u_k - l_k: finite / +inf)
  d_free            the same for a free pair (l = -inf, u = +inf)
  flip_up, flip_dn  the entering variable reaches its own opposite bound before any row blocks it: no basis change, the pair's
                    multiplier enters next
  exit_art_leaves   the basis change in which the artificial variable leaves: solved
  exit_art_flip     the artificial variable reaches 0 unblocked in a flip: solved
  exit_ray          nothing blocks the entering variable and it has no limit of its own
  exit_budget       the pivot budget is used up at the head of the next iteration
  exit_fail         the complement of the leaving variable is in no column

and appends "+tie" when the row was chosen by the tie-break (more than one row inside the ratio window).

It is no reference for values: tests/test_stage_b_transitions_host.py accepts it only with the oracle's status and pivot
count on every node, and with the flips of tests/stage_b_lemke.py.

The batch of a shape is built from three sources: the special classes of tests/stage_b_cases.py, the natural synthetic
nodes FIRST_ID .. FIRST_ID + NATURAL - 1, and the same synthetic nodes with every third row bounded below only and every
third bounded above only (the one-sided pairs, whose p_k enters with self_lim = +inf from the range table).  COVERED names
the ordered pairs its walks take, per shape, over the runs of runs();`exit_art_flip` is in none of them and cannot be: the
artificial variable is nonbasic only in the first iteration, and there the row of the largest violation sits exactly on the
bound it is pushed to (ratio 0) or on the middle of its range (ratio below theta0), so a row always blocks it.

Pure numpy here; the oracle and the GPU are the callers' business."""
import numpy as np

import problems as P
import stage_b_cases as S

INF = np.inf
FIRST_ID, NATURAL = 9000, 60
WS = P.shared_params()
BUDGET_EXTRA = S.BUDGET_EXTRA
SHAPES = [(32, 32), (16, 16), (20, 12)]
EXITS = ("exit_art_leaves", "exit_art_flip", "exit_ray", "exit_budget", "exit_fail")


def runs(n):
    """The (label, parameters, pivot budget in the oracle's count) of the runs that COVERED is taken over."""
    return [("w0", S.W0, 0), ("ws", WS, 0), ("w0 budget", S.W0, n + BUDGET_EXTRA)]


def labelled_walk(Q, R, qd, A, B, l, u, w, piv_tol, feas_tol, max_pivots=0, slack=1e-10):
    """-> dict(status, pivots (Stage B only), flips (as tests/stage_b_lemke.py), kinds: the name of every iteration in order).
    max_pivots counts like the oracle's and the kernel's: the n pivots of the crash included."""
    n, m = qd.shape[0], l.shape[0]
    g = qd + R @ w
    S_ = A @ np.linalg.solve(Q, A.T)
    xb = B @ w - A @ np.linalg.solve(Q, g)
    T = S_.copy()
    lo0, hi0 = l.astype(float).copy(), u.astype(float).copy()
    lo, hi = lo0.copy(), hi0.copy()
    cls = np.where((lo0 == -INF) & (hi0 == INF), 2, 0)
    rng = hi0 - lo0
    sat = np.zeros(m, int)
    VTH, XC = 2 * m, m
    rowvar = np.arange(m)
    colvar = np.concatenate([m + np.arange(m), [VTH]])
    nbval = np.zeros(m + 1)
    tcol = np.zeros(m)
    out = dict(status=4, pivots=0, flips=[], kinds=[])
    viol = np.where(xb < lo, lo - xb, np.where(xb > hi, xb - hi, 0.0))
    theta0 = viol.max()
    if theta0 <= feas_tol:
        out["status"] = 1
        return out
    for k in range(m):
        if xb[k] < lo[k]:
            tgt = lo[k] + (theta0 - (lo[k] - xb[k]))
            if hi[k] < INF:
                tgt = min(tgt, 0.5 * (lo[k] + hi[k]))
            tcol[k] = (tgt - xb[k]) / theta0; xb[k] = tgt
        elif xb[k] > hi[k]:
            tgt = hi[k] - (theta0 - (xb[k] - hi[k]))
            if lo[k] > -INF:
                tgt = max(tgt, 0.5 * (lo[k] + hi[k]))
            tcol[k] = (tgt - xb[k]) / theta0; xb[k] = tgt
    nbval[XC] = theta0
    self_lim, c, sneg, elo, ehi = theta0, XC, True, 0.0, INF
    limit = max_pivots - n if max_pivots > 0 else 50 * (n + m) + 100 - n
    while True:
        if out["pivots"] >= limit:
            out["status"] = 3; out["kinds"].append("exit_budget")
            return out
        cm = tcol.copy() if c == XC else T[:, c].copy()
        gdir = -cm if sneg else cm
        with np.errstate(divide="ignore", invalid="ignore"):
            rc = 1.0 / gdir
            tb = np.where(np.signbit(gdir), lo, hi)
            cnd = (np.abs(gdir) > piv_tol) & (np.abs(tb) < INF)
            dd = np.where(cnd, (tb - xb) * rc, INF)
            d1 = np.where(cnd, dd + slack * np.abs(rc), INF)
        dmax = min(d1.min(), self_lim)
        if dmax == INF:
            out["status"] = 2; out["kinds"].append("exit_ray")
            return out
        bal = dd <= dmax
        if not bal.any():
            xb = xb + (-self_lim if sneg else self_lim) * cm
            ve = colvar[c]
            if ve == VTH:
                out["status"] = 1; out["kinds"].append("exit_art_flip")
                return out
            k = int(ve)
            au = 0 if sneg else 1
            out["flips"].append(+1 if au else -1)
            nbval[c] = hi0[k] if au else lo0[k]
            sat[k] = au
            out["pivots"] += 1
            hit = np.flatnonzero(colvar == m + k)
            if len(hit) == 0:
                out["kinds"].append("exit_fail")
                return out
            out["kinds"].append("flip_up" if au else "flip_dn")
            c = int(hit[0]); sneg = au != 0; self_lim = INF
            elo, ehi = (-INF, 0.0) if au else (0.0, INF)
            continue
        tie = bal.sum() > 1
        if not tie:
            r = int(np.flatnonzero(bal)[0])
        else:
            ag = np.where(bal, np.abs(gdir), -1.0)
            ag[bal & (rowvar == VTH)] = INF
            r = int(np.flatnonzero(bal & (ag == ag.max()))[0])
        suffix = "+tie" if tie else ""
        step = max(dd[r], 0.0)
        leave_val, rcr = tb[r], rc[r]
        inv = -rcr if sneg else rcr
        delta = -step if sneg else step
        vl = int(rowvar[r])
        enter_val = nbval[c] + delta
        row = T[r, :].copy(); px = tcol[r]
        if c == XC:
            px = -1.0
        else:
            row[c] = -1.0
        v = row * inv; vx = px * inv
        tc0 = np.zeros(m) if c == XC else tcol
        xbn = xb + delta * cm; tcn = tc0 - cm * vx
        xbn[r] = enter_val; tcn[r] = -vx
        xb, tcol = xbn, tcn
        T = T - np.outer(cm, v)
        if c != XC:
            T[:, c] = cm * inv
        T[r, :] = -v
        ve = int(colvar[c])
        rowvar[r] = ve; lo[r], hi[r] = elo, ehi
        colvar[c] = vl; nbval[c] = leave_val
        out["pivots"] += 1
        if vl == VTH:
            out["status"] = 1; out["kinds"].append("exit_art_leaves" + suffix)
            return out
        k = vl if vl < m else vl - m
        if vl < m:
            au = 0 if np.signbit(rcr) else 1
            kind = "first" if out["pivots"] == 1 else ("p_hi" if au else "p_lo")
            sat[k] = au; vn = m + k; sneg = au != 0; self_lim = INF
            elo, ehi = (0.0, 0.0) if cls[k] == 2 else ((-INF, 0.0) if au else (0.0, INF))
        else:
            kind = "d_free" if cls[k] == 2 else ("d_two" if rng[k] < INF else "d_one")
            au = sat[k]; vn = k; sneg = au != 0 and cls[k] != 2; self_lim = rng[k]
            elo, ehi = lo0[k], hi0[k]
        hit = np.flatnonzero(colvar == vn)
        if vn == ve or len(hit) == 0:
            out["kinds"].append("exit_fail")
            return out
        out["kinds"].append(kind + suffix)
        c = int(hit[0])


def pairs_of(kinds):
    return {(a, b) for a, b in zip(kinds[:-1], kinds[1:])}


def base(kind):
    return kind.split("+")[0]


# ---- the batch ------------------------------------------------------------------------------------------------------------
_cache = {}


def one_sided(rec):
    """The node with every third row bounded below only and every third bounded above only."""
    Q, R, qd, A, B, l, u = (c.copy() for c in rec)
    k = np.arange(l.shape[0])
    u[k % 3 == 0] = INF; l[k % 3 == 1] = -INF
    return Q, R, qd, A, B, l, u


def batch(n, m):
    """-> (records in math layout (stacked), names: what each node is, in order)."""
    if (n, m) not in _cache:
        recs, names = [], []
        for name in S.class_names(m):
            recs.append(S.special(name, n, m)[0]); names.append(name)
        for i in range(FIRST_ID, FIRST_ID + NATURAL):
            recs.append(P.synth_node(i, n, m, 8)); names.append(f"natural_{i}")
        for i in range(FIRST_ID, FIRST_ID + NATURAL):
            recs.append(one_sided(P.synth_node(i, n, m, 8))); names.append(f"one_sided_{i}")
        _cache[(n, m)] = (tuple(np.stack([r[j] for r in recs]) for j in range(7)), names)
    return _cache[(n, m)]


def padded(n, m, cnt, seed):
    """The batch of (n, m) in front of cnt - len(batch) natural synthetic nodes of another seed: the large launches."""
    key = (n, m, cnt, seed)
    if key not in _cache:
        recs, names = batch(n, m)
        fill = P.synth_nodes(seed, cnt - len(names), n, m, 8)
        _cache[key] = (tuple(np.concatenate([a, b]) for a, b in zip(recs, fill)), names)
    return _cache[key]


def walks(n, m, piv_tol, feas_tol):
    """-> {run label: [walk of every node of the batch, None for the declined `equal` node]}."""
    key = ("walks", n, m, piv_tol, feas_tol)
    if key not in _cache:
        recs, names = batch(n, m)
        _cache[key] = {label: [None if nm == "equal" else labelled_walk(*(c[i] for c in recs), w, piv_tol, feas_tol, mp)
                               for i, nm in enumerate(names)] for label, w, mp in runs(n)}
    return _cache[key]


def covered(n, m, piv_tol, feas_tol):
    got = set()
    for ws in walks(n, m, piv_tol, feas_tol).values():
        for wk in ws:
            if wk is not None:
                got |= pairs_of(wk["kinds"])
    return got


# ---- GPU scenarios: those of tests/stage_b_cases.py that reach another instantiation of the loop, on this batch -------------
# name -> (kind, cnt (0: the batch alone), n, m, seed of the padding)
SCENARIOS = {
    "resident_sym": ("handle", 0, 32, 32, 0),
    "nodes_16": ("nodes", 0, 16, 16, 0),
    "nodes_20_12": ("nodes", 0, 20, 12, 0),
    "explicit_64": ("explicit", 0, 32, 32, 0),
    "budget_32": ("budget", 0, 32, 32, 0),
    "resident_4224_stream": ("handle_llc-1", 4224, 32, 32, 624224),
    "resident_4224_plain": ("handle_llc0", 4224, 32, 32, 624224),
}


def scenario_records(name):
    kind, cnt, n, m, seed = SCENARIOS[name]
    recs, names = padded(n, m, cnt, seed) if cnt else batch(n, m)
    if kind == "budget":                                # (as in tests/stage_b_cases.py: the budget is asked of the fused kernel's nodes)
        keep = [i for i, nm in enumerate(names) if nm != "equal"]
        recs, names = tuple(c[keep] for c in recs), [names[i] for i in keep]
    return recs, names


def run_scenario(engine, name):
    """Runs one scenario on the GPU -> [(label, w, outputs as numpy arrays, max_pivots)], in a fixed order."""
    from qpn_amd import _lib
    kind, _, n, m, seed = SCENARIOS[name]
    recs, names = scenario_records(name)
    cnt = recs[0].shape[0]
    out_runs = []
    if kind.startswith("handle"):
        llc = int(kind.split("llc")[1]) if "llc" in kind else None
        if llc is not None:
            engine.set_option(_lib.OPT_LLC_BUDGET_MB, llc)
        try:
            h = engine.upload_nodes(*S.abi(recs))
            h.set_schedule(0)
            # a computing sweep that fills the crash cache, a reuse sweep of the same parameters, one of other parameters
            for label, w in (("fill w0", S.W0), ("reuse w0", S.W0), ("reuse ws", WS)):
                x = np.zeros((cnt, n + 3))
                out = S._np(h.solve(w, x_out=x)); out["x_out"] = x
                out_runs.append((label, w, out, 0))
            info = h.info()
            assert info["symmetric"] and info["declined"] >= 1, info            # the `equal` node went to the general kernel
            if llc is not None:
                assert info["crash_cached"] and info["crash_streamed"] == (llc < 0), info
            h.close()
        finally:
            if llc is not None:
                engine.set_option(_lib.OPT_LLC_BUDGET_MB, S._default_llc_budget())
    elif kind in ("nodes", "budget"):
        mp = n + BUDGET_EXTRA if kind == "budget" else 0
        o = engine.default_opts(); o.max_pivots = mp
        for label, w in (("w0", S.W0), ("ws", WS)):
            x = np.zeros((cnt, n + 3))
            out = S._np(engine.solve_nodes(*S.abi(recs), w, opts=o, x_out=x)); out["x_out"] = x
            out_runs.append((label, w, out, mp))
    elif kind == "explicit":
        from qpn_amd.engine import colmajor
        for label, w in (("w0", S.W0), ("ws", WS)):
            M, q, lo, hi, kd = P.reduced_blocks(*recs, w)
            out = S._np(engine.solve_avi_batch(colmajor(M), q, lo, hi, kind=kd)); out["x_out"] = out["z"][:, :n].copy()
            out_runs.append((label, w, out, 0))
    else:
        raise KeyError(kind)
    return out_runs


# ---- the ordered pairs of kinds that the batch of each shape covers (tests/test_stage_b_transitions_host.py holds the batch
# to them: a batch that lost one fails there, before it fails to test anything on the device) --------------------------------
COVERED = {
    (32, 32): (
        ("d_one", "exit_art_leaves"), ("d_one", "p_hi"), ("d_one", "p_lo"), ("d_two", "d_one"), ("d_two", "d_two"),
        ("d_two", "exit_art_leaves"), ("d_two", "exit_budget"), ("d_two", "flip_dn"), ("d_two", "flip_up"),
        ("d_two", "p_hi"), ("d_two", "p_lo"), ("first", "exit_art_leaves"), ("first", "exit_art_leaves+tie"),
        ("first", "p_hi"), ("first", "p_lo"), ("first+tie", "exit_art_leaves"), ("first+tie", "p_hi"),
        ("first+tie", "p_lo"), ("flip_dn", "exit_art_leaves"), ("flip_up", "d_two"), ("flip_up", "p_hi"), ("p_hi", "d_one"),
        ("p_hi", "d_two"), ("p_hi", "exit_art_leaves"), ("p_hi", "exit_budget"), ("p_hi", "exit_ray"), ("p_hi", "p_hi"),
        ("p_hi", "p_lo"), ("p_lo", "d_one"), ("p_lo", "d_two"), ("p_lo", "exit_art_leaves"), ("p_lo", "exit_budget"),
        ("p_lo", "p_hi"), ("p_lo", "p_lo"),
    ),
    (16, 16): (
        ("d_one", "exit_art_leaves"), ("d_one", "exit_budget"), ("d_one", "p_hi"), ("d_one", "p_lo"), ("d_two", "d_two"),
        ("d_two", "exit_art_leaves"), ("d_two", "exit_budget"), ("d_two", "flip_dn"), ("d_two", "flip_up"),
        ("d_two", "p_hi"), ("d_two", "p_lo"), ("first", "exit_art_leaves"), ("first", "exit_art_leaves+tie"),
        ("first", "p_hi"), ("first", "p_lo"), ("first+tie", "exit_art_leaves"), ("first+tie", "p_hi"),
        ("first+tie", "p_lo"), ("flip_dn", "d_two"), ("flip_dn", "p_lo"), ("flip_up", "exit_art_leaves"),
        ("flip_up", "p_hi"), ("flip_up", "p_lo"), ("p_hi", "d_one"), ("p_hi", "d_two"), ("p_hi", "exit_art_leaves"),
        ("p_hi", "exit_budget"), ("p_hi", "exit_ray"), ("p_hi", "p_hi"), ("p_hi", "p_lo"), ("p_lo", "d_one"),
        ("p_lo", "d_two"), ("p_lo", "exit_art_leaves"), ("p_lo", "exit_budget"), ("p_lo", "p_hi"), ("p_lo", "p_lo"),
    ),
    (20, 12): (
        ("d_one", "exit_art_leaves"), ("d_one", "p_lo"), ("d_two", "exit_art_leaves"), ("d_two", "exit_budget"),
        ("d_two", "flip_dn"), ("d_two", "flip_up"), ("d_two", "p_hi"), ("d_two", "p_lo"), ("first", "exit_art_leaves"),
        ("first", "exit_art_leaves+tie"), ("first", "p_hi"), ("first", "p_lo"), ("first+tie", "exit_art_leaves"),
        ("first+tie", "p_hi"), ("first+tie", "p_lo"), ("flip_dn", "d_two"), ("flip_up", "p_lo"), ("p_hi", "d_one"),
        ("p_hi", "d_two"), ("p_hi", "exit_art_leaves"), ("p_hi", "exit_budget"), ("p_hi", "exit_ray"), ("p_hi", "p_hi"),
        ("p_hi", "p_lo"), ("p_lo", "d_one"), ("p_lo", "d_two"), ("p_lo", "exit_art_leaves"), ("p_lo", "exit_budget"),
        ("p_lo", "exit_ray"), ("p_lo", "p_hi"), ("p_lo", "p_lo"),
    ),
}
