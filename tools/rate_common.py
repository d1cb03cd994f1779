"""What the rate tools of the polyhedral entries share (lp_rate, subset_rate, implicit_bounds_rate, exemplar_rate,
interior_members_rate): the import path, the host clock around a synchronise, the alternating rounds with their JSON lines, the
upload of a call's arrays, the engine with a method hidden (polyhedra.without) and the stacks check_convexity sends."""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import qpn_amd  # noqa: E402
from qpn_amd import algorithm, examples, polyhedra  # noqa: E402
from qpn_amd.polyhedra import without  # noqa: E402,F401


def emit(**line):
    print(json.dumps(line), flush=True)


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def report(what, routes, rounds, medians=True, per=lambda s: {}, **info):
    """`rounds` rounds, the routes [(name, fn)] alternating in each: one line per measurement (with per(seconds) added) and one
    with the medians per route."""
    times = {name: [] for name, _ in routes}
    for rnd in range(rounds):
        for name, fn in routes:
            s = timed(fn)
            times[name].append(s)
            emit(what=what, route=name, round=rnd, seconds=s, **per(s), **info)
    if medians:
        emit(what=what, medians={name: float(np.median(v)) for name, v in times.items()}, **info)


def on_device(eng, arrays):
    import torch
    return tuple(torch.as_tensor(np.ascontiguousarray(a), device=f"cuda:{eng.device}") for a in arrays)


def quiet_solve(net, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return algorithm.solve(net, *args, **kw)


def convexity_stacks(engine, pairs):
    """The largest batch of constraint stacks check_convexity sends to implicit_bounds_batch during one solve() of `pairs`
    synthetic pairs of (16, 16)."""
    seen = []
    real = polyhedra.implicit_bounds_batch

    def capture(polys, engine, tol=1e-4, **kw):
        seen.append([tuple(np.asarray(v, dtype=np.float64) for v in p) for p in polys])
        return real(polys, engine, tol=tol, **kw)

    polyhedra.implicit_bounds_batch = capture
    try:
        quiet_solve(examples.setup("synthetic_pairs", pairs=pairs, n=16, m=16, check_convexity=True), engine=engine)
    finally:
        polyhedra.implicit_bounds_batch = real
    return max(seen, key=len)
