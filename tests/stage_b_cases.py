"""Seeded nodes that walk the exits and joins of the Stage B pivot loop of the fused 32-class kernel (the Lemke loop of
csrc/qpn_avi_schur.hip), the batches that reach its instantiations, and what each class must show in the outputs.

A special node is a synthetic node whose constraint bounds are opened to +-1e6 and whose chosen rows are then placed against
s0 = A x0 + B w0, the constraint values at the unconstrained minimiser x0 = -Q^-1 (qd + R w0): Stage B starts from exactly
these values, so a row's bounds decide what the loop does with it.

  feasible        nothing violated: the loop body never runs, pivots == n
  row_reg_0 .. 7  one row k violated by 1, with k = 16 Ib + 4 g + lq chosen so that the pivot row is read from -- and written
                  back to -- tile register 4 Ib + g = 0 .. 7: the first pivot enters the extra (covering) column and p_k
                  leaves, the second enters d_k from dictionary column k (tile column 0 for k < 16, 1 for k >= 16) and the
                  artificial variable leaves.  pivots == n + 2, lambda_k is the only multiplier
  one_lo, one_hi  the same with the other bound infinite, one case per side
  free_pair       a row with l = -inf, u = +inf (class 2) next to two violated rows: its multiplier stays 0
  tie             two bitwise-equal constraint rows with bitwise-equal bounds, both violated by 1: the first ratio test ties
                  exactly, and the loop takes the tie-break path.  Both rows end on their bound
  tie_artificial  two bitwise-equal rows, the first violated by 1, the second with its UPPER bound at the first one's lower
                  bound: in the second pivot the second row reaches its bound when the artificial variable reaches 0, and the
                  artificial variable must win.  pivots == n + 2, only the first row's multiplier
  flips           every row violated by (1 + k / 64) / 20, even rows from below and odd rows from above, ranges of 0.005: variables enter and
                  reach their own opposite bound first (no basis change), at least once from lo to hi and once from hi to lo.
                  The outputs do not tell a flip from a basis change (`pivots` counts both), so presence is shown by the walk
                  of tests/stage_b_lemke.py: it counts them apart, and it is accepted only with the oracle's pivot count --
                  the GPU test inherits presence through pivots equal to the oracle's.  In the outputs: a row of each
                  direction ends on the bound OPPOSITE to the violated one
  many            every row k violated from below by 1 + k / 64, ranges of 1: long solves (the node of the pivot budget)
  ray             two bitwise-equal rows with contradictory bounds: status QPN_RAY_TERM
  equal           a row with l == u: the fused kernel declines the node, the general kernel solves it

Rows are taken modulo m, so the same classes exist for n = m = 16 and the ragged (20, 12) shape (row_reg_4 .. 7 need m > 16
and are left out below that).  Pure numpy here; the oracle and the GPU are the callers' business."""
import numpy as np

import problems as P

OPEN = 1e6
W0 = np.random.default_rng(77).standard_normal(8)
KEYS = ("z", "status", "resid", "pivots", "active", "x_out")
SUCCESS, RAY_TERM, MAX_ITERS = 1, 2, 3
FIRST_ID = 9000
# the synthetic node the `flips` class is made from, per shape: one whose walk through the loop (tests/stage_b_lemke.py) takes
# the bound-flip branch in BOTH directions, with the oracle's pivot count and multipliers of a few units
# (tests/test_stage_b_cases_host.py asserts all of that); every other class is made from FIRST_ID
FLIP_NODE = {(32, 32): 9079, (16, 16): 9187, (20, 12): 9090, (20, 20): 9080}


def reg_row(j):
    """A row whose tile register is j (= 4 Ib + g), with the lane group lq varying over the registers."""
    return 16 * (j >> 2) + 4 * (j & 3) + (j & 3)


def _open(node_id, n, m, twin=None):
    """The opened node and s0; twin = (a, b): row b of Ad and B becomes a bitwise copy of row a."""
    Q, R, qd, A, B, l, u = P.synth_node(node_id, n, m, 8)
    if twin is not None:
        A[twin[1]] = A[twin[0]]; B[twin[1]] = B[twin[0]]
    x0 = -np.linalg.solve(Q, qd + R @ W0)
    s0 = A @ x0 + B @ W0
    return [Q, R, qd, A, B, np.full(m, -OPEN), np.full(m, OPEN)], s0


def class_names(m):
    regs = [f"row_reg_{j}" for j in range(8) if reg_row(j) < m]
    return ["feasible"] + regs + ["one_lo", "one_hi", "free_pair", "tie", "tie_artificial", "flips", "many", "ray", "equal"]


def special(name, n, m):
    """-> (record (Q, R, qd, A, B, l, u) in math layout, meta: the rows the class is about)."""
    node_id = FLIP_NODE[(n, m)] if name == "flips" else FIRST_ID
    a, b = 5 % m, 6 % m
    if name in ("tie", "tie_artificial", "ray"):
        rec, s0 = _open(node_id, n, m, twin=(a, b))
        assert s0[a] == s0[b]
    else:
        rec, s0 = _open(node_id, n, m)
    l, u = rec[5], rec[6]
    meta = {}
    if name == "feasible":
        pass
    elif name.startswith("row_reg_"):
        k = reg_row(int(name[-1])); l[k] = s0[k] + 1.0; u[k] = s0[k] + 2.0; meta["k"] = k
    elif name == "one_lo":
        k = 3 % m; l[k] = s0[k] + 1.0; u[k] = np.inf; meta["k"] = k
    elif name == "one_hi":
        k = 19 % m; l[k] = -np.inf; u[k] = s0[k] - 1.0; meta["k"] = k
    elif name == "free_pair":
        rows = [3 % m, 20 % m]; f = 7 % m
        assert len({f, *rows}) == 3
        for k in rows:
            l[k] = s0[k] + 1.0; u[k] = s0[k] + 2.0
        l[f] = -np.inf; u[f] = np.inf
        meta.update(rows=rows, free=f)
    elif name == "tie":
        for k in (a, b):
            l[k] = s0[a] + 1.0; u[k] = s0[a] + 2.0
        meta.update(a=a, b=b)
    elif name == "tie_artificial":
        l[a] = s0[a] + 1.0; u[a] = s0[a] + 2.0; u[b] = s0[a] + 1.0
        meta.update(a=a, b=b)
    elif name == "ray":
        l[a] = s0[a] + 1.0; u[a] = s0[a] + 2.0; l[b] = s0[a] - 2.0; u[b] = s0[a] - 1.0
        meta.update(a=a, b=b)
    elif name == "flips":
        up = np.arange(m) % 2 == 0
        # (violations that differ: no tie in the first ratio test; small ones: the multipliers grow with them, and with the
        # multipliers the absolute deviation from the oracle that the same relative error makes)
        v = 0.05 * (1.0 + np.arange(m) / 64.0)
        l[:] = np.where(up, s0 + v, s0 - v - 0.005); u[:] = np.where(up, s0 + v + 0.005, s0 - v)
        meta["up"] = up
    elif name == "many":
        v = 1.0 + np.arange(m) / 64.0
        l[:] = s0 + v; u[:] = s0 + v + 1.0
    elif name == "equal":
        k = 4 % m; l[k] = u[k] = s0[k] + 0.5; meta["k"] = k
    else:
        raise KeyError(name)
    return rec, meta


def check_marker(name, rec, meta, out, i, n):
    """What class `name` must show in item i of the outputs `out` (of the oracle or of the GPU) at the parameters W0."""
    Q, R, qd, A, B, l, u = rec
    m = l.shape[0]
    st, piv, z = int(out["status"][i]), int(out["pivots"][i]), np.asarray(out["z"][i])
    lam = z[n:n + m]; nz = list(np.flatnonzero(lam != 0.0))
    s = A @ z[:n] + B @ W0
    if name == "ray":
        assert st == RAY_TERM, (name, st)
        assert np.array_equal(A[meta["a"]], A[meta["b"]]) and l[meta["a"]] > u[meta["b"]]
        return
    assert st == SUCCESS, (name, st)
    if name == "feasible":
        assert piv == n and nz == [], (name, piv, nz)
    elif name.startswith("row_reg_") or name in ("one_lo", "one_hi"):
        assert piv == n + 2 and nz == [meta["k"]], (name, piv, nz)
    elif name == "free_pair":
        assert l[meta["free"]] == -np.inf and u[meta["free"]] == np.inf
        assert nz == sorted(meta["rows"]) and piv > n + 2, (name, piv, nz)
    elif name == "tie":
        a, b = meta["a"], meta["b"]
        assert np.array_equal(A[a], A[b]) and np.array_equal(B[a], B[b]) and l[a] == l[b] and u[a] == u[b]
        assert abs(s[a] - l[a]) <= 1e-9 and abs(s[b] - l[b]) <= 1e-9 and set(nz) <= {a, b} and nz, (name, s[a] - l[a], nz)
    elif name == "tie_artificial":
        a, b = meta["a"], meta["b"]
        assert np.array_equal(A[a], A[b]) and u[b] == l[a]
        assert piv == n + 2 and nz == [a] and abs(s[b] - u[b]) <= 1e-9, (name, piv, nz, s[b] - u[b])
    elif name == "flips":
        up = meta["up"]
        crossed_up = up & (np.abs(s - u) <= 1e-9); crossed_down = ~up & (np.abs(s - l) <= 1e-9)
        assert crossed_up.any() and crossed_down.any(), (name, crossed_up.sum(), crossed_down.sum())
    elif name == "many":
        assert len(nz) >= min(20, m // 2) and piv - n >= len(nz), (name, piv, len(nz))
    elif name == "equal":
        k = meta["k"]
        assert l[k] == u[k] and abs(s[k] - l[k]) <= 1e-9, (name, s[k] - l[k])


# ---- batches ------------------------------------------------------------------------------------------------------------
_cache = {}


def batch(cnt, n, m, seed, leave_out=()):
    """-> (records in math layout (stacked), where: {class: node index}).  Class j sits at node 2 + 5 j."""
    key = (cnt, n, m, seed, tuple(leave_out))
    if key not in _cache:
        Q, R, qd, A, B, l, u = (c.copy() for c in P.synth_nodes(seed, cnt, n, m, 8))
        where = {}
        for j, name in enumerate(nm for nm in class_names(m) if nm not in leave_out):
            i = 2 + 5 * j
            assert i < cnt
            rec, _ = special(name, n, m)
            Q[i], R[i], qd[i], A[i], B[i], l[i], u[i] = rec
            where[name] = i
        _cache[key] = ((Q, R, qd, A, B, l, u), where)
    return _cache[key]


def abi(recs):
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u = recs
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]


def oracle_solve(oracle, recs, w, idx=None, max_pivots=0):
    Q, R, qd, A, B, l, u = recs if idx is None else tuple(c[idx] for c in recs)
    M, q, lo, hi, kind = P.reduced_blocks(Q, R, qd, A, B, l, u, w)
    o = oracle.default_opts(); o.max_pivots = max_pivots
    return oracle.solve_avi_batch(M, q, lo, hi, kind=kind, opts=o)


W1 = np.random.default_rng(78).standard_normal(8)
BUDGET_EXTRA = 5            # pivot budget of the max_pivots scenario: n + 5, between the two-pivot classes and `many`

# name -> (kind, cnt, n, m, seed)
SCENARIOS = {
    "resident_96_sym": ("handle", 96, 32, 32, 610096),
    "resident_96_asym": ("handle_asym", 96, 32, 32, 610096),
    "nodes_16": ("nodes", 96, 16, 16, 610016),
    "nodes_20_12": ("nodes", 96, 20, 12, 612012),
    "explicit_64": ("explicit", 96, 32, 32, 610096),
    "explicit_40": ("explicit", 96, 20, 20, 612020),
    "budget_96": ("budget", 96, 32, 32, 610096),
    "resident_4224_stream": ("handle_llc-1", 4224, 32, 32, 614224),
    "resident_4224_plain": ("handle_llc0", 4224, 32, 32, 614224),
}


def scenario_records(name):
    kind, cnt, n, m, seed = SCENARIOS[name]
    recs, where = batch(cnt, n, m, seed, leave_out=("equal",) if kind == "budget" else ())
    if kind == "handle_asym":
        Q = recs[0].copy(); Q[cnt - 1, 0, 1] += 1e-3            # one Qd that is not bitwise symmetric: the whole handle leaves the symmetric route
        recs = (Q,) + tuple(recs[1:])
    return recs, where


def _np(res):
    return {k: np.array(v.cpu() if hasattr(v, "cpu") else v) for k, v in res.items() if v is not None}


def run_scenario(engine, name):
    """Runs one scenario on the GPU -> [(label, w, outputs as numpy arrays, max_pivots)], in a fixed order."""
    from qpn_amd import _lib
    kind, cnt, n, m, seed = SCENARIOS[name]
    recs, where = scenario_records(name)
    runs = []
    if kind.startswith("handle"):
        llc = int(kind.split("llc")[1]) if "llc" in kind else None
        if llc is not None:
            engine.set_option(_lib.OPT_LLC_BUDGET_MB, llc)
        try:
            h = engine.upload_nodes(*abi(recs))
            h.set_schedule(0)
            # a computing sweep that fills the crash cache, a reuse sweep of the same parameters, one of other parameters
            for label, w in (("fill w0", W0), ("reuse w0", W0), ("reuse w1", W1)):
                x = np.zeros((cnt, n + 3))
                out = _np(h.solve(w, x_out=x)); out["x_out"] = x
                runs.append((label, w, out, 0))
            info = h.info()
            assert info["symmetric"] == (kind != "handle_asym"), info
            assert info["declined"] >= 1, info            # the `equal` node went to the general kernel
            if llc is not None:
                assert info["crash_cached"] and info["crash_streamed"] == (llc < 0), info
            h.close()
        finally:
            if llc is not None:
                engine.set_option(_lib.OPT_LLC_BUDGET_MB, _default_llc_budget())
    elif kind in ("nodes", "budget"):
        mp = n + BUDGET_EXTRA if kind == "budget" else 0
        o = engine.default_opts(); o.max_pivots = mp
        for label, w in (("w0", W0), ("w1", W1)):
            x = np.zeros((cnt, n + 3))
            out = _np(engine.solve_nodes(*abi(recs), w, opts=o, x_out=x)); out["x_out"] = x
            runs.append((label, w, out, mp))
    elif kind == "explicit":
        from qpn_amd.engine import colmajor
        for label, w in (("w0", W0), ("w1", W1)):
            M, q, lo, hi, kd = P.reduced_blocks(*recs, w)
            out = _np(engine.solve_avi_batch(colmajor(M), q, lo, hi, kind=kd)); out["x_out"] = out["z"][:, :n].copy()
            runs.append((label, w, out, 0))
    else:
        raise KeyError(kind)
    return runs


def _default_llc_budget():
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadraticprogramnetworks.jl_amd", "csrc", "qpn_internal.h")
    mt = re.search(r"#ifndef QPN_LLC_BUDGET_MB\s*\n#define QPN_LLC_BUDGET_MB\s+(-?\d+)\s*\n#endif", open(src).read())
    assert mt
    return int(mt.group(1))


def digests(out):
    import hashlib
    return {k: hashlib.sha256(np.ascontiguousarray(out[k]).tobytes()).hexdigest() for k in KEYS}
