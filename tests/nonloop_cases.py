"""Seeded batches for the code of the fused 32-class kernel (csrc/qpn_avi_schur.hip) OUTSIDE the Stage B pivot loop: the reuse
body's first round of loads (the LDS-DMA of Ad among them) and its replay, the c sweep, the read-back, the post-check and the
stores.  Shape n = m = 32 throughout, resident handles, and what each scenario runs on the GPU.  Pure numpy up to `run`;
tests/test_gpu_nonloop_paths.py and tests/golden/make_nonloop_paths_record.py are the callers.

  layout_4160, layout_64   Ad holds distinct integers, A[r][c] = 1 + r + 32 c -- in memory (column-major) the running index of
                           the entry -- scaled by a power of two per node; Qd = I + a bitwise symmetric perturbation; B small and
                           dense.  A column of Ad that lands anywhere but in its own place of the LDS block buffer changes c, the
                           post-check and with them resid and active.  4 160 = 4 096 + 64 nodes is the smallest batch whose reuse
                           sweeps take the mixed, staggered instantiations; 64 nodes take the plain ones.  Four handles over the
                           same records -- QPN_OPT_LLC_BUDGET_MB -1 (reuse sweeps stream the crash cache) and 0 (none does),
                           QPN_OPT_CRASH_CACHE off (every sweep computes), and a fresh handle per sweep (a filling sweep)
  params_p                 p = 0, 1, 7, 8, 9, 16 parameters (q = [qd + R w; B w] is summed eight terms at a time), dense B, and w
                           once shared by all nodes and once one row per node, the rows strided
  checks                   synthetic nodes whose bounds are infinite below, above, on both sides (every fourth node each) or
                           finite; the special nodes of tests/stage_b_cases.py with all multipliers zero (`feasible`) and with
                           exactly one nonzero multiplier in tile column 0 (`row_reg_1`: row 5) or tile column 1 (`row_reg_5`:
                           row 21); and the same sweep with check_tol = 0, under which the post-check counts a violation on a
                           solved node and turns its status into QPN_FAILURE
"""
import hashlib

import numpy as np

import problems as P
import stage_b_cases as S

N = 32
KEYS = S.KEYS
SUCCESS, FAILURE = 1, 4
W0 = S.W0
PARAM_COUNTS = (0, 1, 7, 8, 9, 16)
LAYOUT_COUNTS = (4160, 64)
CHECK_COUNT = 64
CHECK_SPECIALS = {"feasible": 9, "row_reg_1": 22, "row_reg_5": 43}
_cache = {}


def layout_records(cnt):
    """Records in math layout; Ad as described above."""
    key = ("layout", cnt)
    if key not in _cache:
        Q, R, qd, A, B, l, u = (c.copy() for c in P.synth_nodes(720000, cnt, N, N, 8))
        rng = np.random.default_rng(7200 + cnt)
        r, c = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
        base = (1 + r + 32 * c).astype(np.float64)
        for i in range(cnt):
            G = rng.standard_normal((N, N))
            Q[i] = np.eye(N) + 0.03125 * (G + G.T)              # bitwise symmetric: a + b == b + a
            A[i] = base * 2.0 ** -(8 + i % 3)
        B[:] = 0.02 * rng.standard_normal(B.shape)
        _cache[key] = (Q, R, qd, A, B, l, u)
    return _cache[key]


def param_records(p):
    key = ("params", p)
    if key not in _cache:
        Q, R, qd, A, B, l, u = (c.copy() for c in P.synth_nodes(730000 + 100 * p, 64, N, N, p))
        B[:] = 0.05 * np.random.default_rng(7300 + p).standard_normal(B.shape)
        _cache[key] = (Q, R, qd, A, B, l, u)
    return _cache[key]


def param_w(p):
    """-> (shared (p,), per node (64, p) as a view with row stride p + 3)."""
    rng = np.random.default_rng(7400 + p)
    shared = rng.standard_normal(p)
    wide = rng.standard_normal((64, p + 3))
    return shared, wide[:, :p]


def check_records():
    if "checks" not in _cache:
        Q, R, qd, A, B, l, u = (c.copy() for c in P.synth_nodes(740000, CHECK_COUNT, N, N, 8))
        for i in range(CHECK_COUNT):
            if i % 4 == 1:
                l[i] = -np.inf
            elif i % 4 == 2:
                u[i] = np.inf
            elif i % 4 == 3:
                l[i] = -np.inf; u[i] = np.inf
        for name, i in CHECK_SPECIALS.items():
            rec, _ = S.special(name, N, N)
            Q[i], R[i], qd[i], A[i], B[i], l[i], u[i] = rec
        _cache["checks"] = (Q, R, qd, A, B, l, u)
    return _cache["checks"]


def digests(out):
    return {k: hashlib.sha256(np.ascontiguousarray(out[k]).tobytes()).hexdigest() for k in KEYS}


def _solve(h, w, opts=None):
    x = np.zeros((h.batch, N + 3))
    out = S._np(h.solve(w, opts=opts, x_out=x))
    out["x_out"] = x
    return out


def _handle(engine, recs):
    h = engine.upload_nodes(*S.abi(recs))
    h.set_schedule(0)                       # natural order: launch position = node index
    return h


def run_layout(engine, cnt):
    """-> [(label, outputs)]: per sweep the four handles' outputs, in the order stream, plain, off, fresh."""
    from qpn_amd import _lib
    recs = layout_records(cnt)
    rng = np.random.default_rng(cnt)
    runs = []

    def budget(v):
        engine.set_option(_lib.OPT_LLC_BUDGET_MB, v)

    stream, plain, off = (_handle(engine, recs) for _ in range(3))
    try:
        for s in range(3):
            w = W0 if s == 0 else rng.standard_normal(8)
            budget(-1)
            runs.append((f"sweep {s}/stream", _solve(stream, w)))
            info = stream.info()
            assert info["symmetric"] and info["crash_cached"] and info["crash_streamed"] == (s > 0), info
            budget(0)
            runs.append((f"sweep {s}/plain", _solve(plain, w)))
            info = plain.info()
            assert info["crash_cached"] and not info["crash_streamed"], info
            engine.set_option(_lib.OPT_CRASH_CACHE, 0)
            try:
                runs.append((f"sweep {s}/off", _solve(off, w)))
                assert not off.info()["crash_cached"]
            finally:
                engine.set_option(_lib.OPT_CRASH_CACHE, 1)
            fresh = _handle(engine, recs)
            runs.append((f"sweep {s}/fresh", _solve(fresh, w)))
            fresh.close()
    finally:
        budget(S._default_llc_budget())
        for h in (stream, plain, off):
            h.close()
    return runs


def run_params(engine, p):
    """-> [(label, outputs)]: a filling and a reuse sweep with the shared w, then the same with one strided row of w per node."""
    recs = param_records(p)
    shared, rows = param_w(p)
    assert rows.strides[0] == 8 * (p + 3)
    runs = []
    h = _handle(engine, recs)
    try:
        for label, w in (("shared/fill", shared), ("shared/reuse", shared), ("rows/reuse", rows), ("rows/reuse again", rows)):
            runs.append((label, _solve(h, w)))
        assert h.info()["crash_cached"]
    finally:
        h.close()
    return runs


def run_checks(engine):
    """-> [(label, outputs)]: fill and reuse with the default tolerances, then a reuse sweep with check_tol = 0."""
    recs = check_records()
    runs = []
    h = _handle(engine, recs)
    try:
        runs.append(("fill", _solve(h, W0)))
        runs.append(("reuse", _solve(h, W0)))
        o = engine.default_opts(); o.check_tol = 0.0
        runs.append(("reuse, check_tol 0", _solve(h, W0, opts=o)))
        assert h.info()["crash_cached"]
    finally:
        h.close()
    return runs


def scenarios():
    """name -> function of the engine that runs it."""
    out = {}
    for cnt in LAYOUT_COUNTS:
        out[f"layout_{cnt}"] = (lambda e, c=cnt: run_layout(e, c))
    for p in PARAM_COUNTS:
        out[f"params_{p}"] = (lambda e, q=p: run_params(e, q))
    out["checks"] = run_checks
    return out
