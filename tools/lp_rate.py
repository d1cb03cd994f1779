"""Rates of the polyhedral LPs on one GPU: the node-AVI route (LPs as nodes with Q = 0, what an engine
without solve_lps takes), qpn_solve_lps in host mode and in device mode.

  stacks     implicit_bounds_batch over the constraint stacks that check_convexity sends for `--pairs` synthetic pairs of (16, 16)
             (captured from one solve()), AVI route and LP route, and the bare solve_lps call over the same jobs in both modes
  gauss      `--polys` Gaussian polyhedra of 48 rows in 24 variables, every (row, sign) a job: solve_lps in both modes, and the
             AVI route on the first `--avi-polys` of them (it builds one padded copy of the polyhedron per job)
  solve      algorithm.solve() on the pairs with check_convexity on and off

In a checkout whose engine has no solve_lps (the commit before this solver: copy this file there) only the AVI route and `solve`
run, so one job can alternate the two checkouts.  Prints one JSON line per measurement.
usage: python tools/lp_rate.py [--pairs 200] [--polys 2000] [--avi-polys 100] [--reps 3]"""
import argparse
import time

import numpy as np

from rate_common import convexity_stacks, emit, examples, on_device, polyhedra, qpn_amd, quiet_solve, without
from qpn_amd.engine import colmajor


def median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def row_jobs(A, l, u):
    """A pack of polyhedra of one shape -> (Ac, l, u, poly_of, obj_row, obj_sign): every (row, sign) a job."""
    B, r, _ = A.shape
    return (colmajor(A), l, u, np.repeat(np.arange(B), 2 * r).astype(np.int32), np.tile(np.repeat(np.arange(r), 2), B).astype(np.int32),
            np.tile([1, -1], B * r).astype(np.int32))


def bare_calls(eng, what, trips, reps, has_lps):
    if not has_lps:
        return
    import torch
    host = [row_jobs(A, l, u) for _, _, A, l, u in polyhedra.pack_by_shape(trips)[0]]
    jobs = sum(len(p[3]) for p in host)
    dev = [on_device(eng, h) for h in host]

    def run(args):
        for Ac, l, u, po, row, sg in args:
            eng.solve_lps(Ac, l, u, po, obj_row=row, obj_sign=sg)
        torch.cuda.synchronize()

    for mode, args in (("host", host), ("device", dev)):
        s = median_time(lambda: run(args), reps)
        emit(what=what, route="solve_lps_" + mode, jobs=jobs, calls=len(args), median_s=s, jobs_per_s=jobs / s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--polys", type=int, default=2000)
    ap.add_argument("--avi-polys", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    eng = qpn_amd.default_engine(0)
    has_lps = callable(getattr(eng, "solve_lps", None))
    plain = without(eng, "solve_lps")                       # (the host functions take the node-AVI route)
    emit(what="library", path=qpn_amd._lib.LIB_PATH, has_solve_lps=bool(has_lps))

    # (a) the stacks of check_convexity
    real = polyhedra.implicit_bounds_batch
    stacks = convexity_stacks(plain, a.pairs)
    shapes = sorted({t[0].shape for t in stacks})
    for route, e in (("avi", plain),) + ((("lp", eng),) if has_lps else ()):
        s = median_time(lambda: real(stacks, e), a.reps)
        emit(what="stacks_implicit_bounds", route=route, polys=len(stacks), shapes=shapes[:4], median_s=s)
    bare_calls(eng, "stacks_rows", stacks, a.reps, has_lps)

    # (b) Gaussian polyhedra, row objectives
    rng = np.random.default_rng(0)
    A = rng.standard_normal((a.polys, 48, 24))
    s0 = np.einsum("brd,bd->br", A, rng.standard_normal((a.polys, 24)))
    gauss = [(A[b], s0[b] - np.abs(rng.standard_normal(48)), s0[b] + np.abs(rng.standard_normal(48))) for b in range(a.polys)]
    bare_calls(eng, "gauss_48x24_rows", gauss, a.reps, has_lps)
    few = gauss[:a.avi_polys]
    s = median_time(lambda: real(few, plain), 1)
    emit(what="gauss_48x24_implicit_bounds", route="avi", polys=len(few), jobs=96 * len(few), median_s=s, jobs_per_s=96 * len(few) / s)
    if has_lps:
        s = median_time(lambda: real(few, eng), 1)
        emit(what="gauss_48x24_implicit_bounds", route="lp", polys=len(few), jobs=96 * len(few), median_s=s, jobs_per_s=96 * len(few) / s)

    # (c) solve() with and without the check
    for check in (False, True):
        for route, e in (("avi", plain),) + ((("lp", eng),) if has_lps else ()):
            if not check and route == "lp":
                continue
            t0 = time.perf_counter()
            r = quiet_solve(examples.setup("synthetic_pairs", pairs=a.pairs, n=16, m=16, check_convexity=check), engine=e)
            dt = time.perf_counter() - t0
            emit(what="solve", pairs=a.pairs, n=16, m=16, check_convexity=check, route=route if check else "-", solved=bool(r["solved"]), seconds=dt)


if __name__ == "__main__":
    main()
