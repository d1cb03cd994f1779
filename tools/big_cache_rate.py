#!/usr/bin/env python3
"""Developer aid: what a sweep over resident LARGE records costs with and without the crash cache of the large class
(QPN_OPT_CRASH_CACHE_BIG).  The same records go on two handles in one process, one swept with the option
at 1 and one with it at 0; w walks, and at every w both handles are swept, one after the other, each between two
synchronisations under a host clock.  Reported per case (medians; the uncached sweep's own max - min is the yardstick's spread):

  uncached   the option-0 handle
  reuse      the option-1 handle once its cache is filled
  fill       the first sweep of a fresh handle with the option at 1 (it also allocates the cache), FILLS of them
  refill     the sweep after an update of Ad on the option-1 handle (the cache is dropped, its memory stays)
  pairwise   uncached - reuse at the same w (Stage B's cost moves with w on both handles alike)

Cases: config 5's records (512 x (256, 256, 8)), an asymmetric copy of them (the Lemke kernel alone: every node pays the copy
of S), and 512 x (144, 16, 8).  Every timed pair of sweeps is also compared bit for bit.
Usage: python tools/big_cache_rate.py [sym] [asym] [small]   (NODES=512 WARM=8 SWEEPS=40 FILLS=5)"""
import os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np, torch
import qpn_amd
import problems as P
from qpn_amd.engine import colmajor
from qpn_amd._lib import OPT_CRASH_CACHE_BIG

cases = sys.argv[1:] or ["sym", "asym", "small"]
NODES = int(os.environ.get("NODES", "512")); WARM = int(os.environ.get("WARM", "8"))
SWEEPS = int(os.environ.get("SWEEPS", "40")); FILLS = int(os.environ.get("FILLS", "5"))
eng = qpn_amd.Engine(0)
t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def sweep(nodes, opt, w):
    eng.set_option(OPT_CRASH_CACHE_BIG, opt)
    torch.cuda.synchronize(); eng.synchronize()
    t0 = time.perf_counter()
    res = nodes.solve(w)
    torch.cuda.synchronize(); eng.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def run(tag, n, m, p, asym):
    Q, R_, qd, A, B, l, u = P.synth_nodes(0, NODES, n, m, p)
    if asym:
        K = np.random.default_rng(5).standard_normal(Q.shape) * 0.02
        Q = Q + (K - K.transpose(0, 2, 1))
    rec = [t(colmajor(Q)), t(colmajor(R_)), t(qd), t(colmajor(A)), t(colmajor(B)), t(l), t(u)]
    rng = np.random.default_rng(1)
    ws = [t(rng.standard_normal(p)) for _ in range(WARM + SWEEPS)]
    on, off = eng.upload_nodes(*rec), eng.upload_nodes(*rec)
    t_on, t_off, same, solved = [], [], True, True
    for k, w in enumerate(ws):
        a_ms, a = sweep(on, 1, w)
        b_ms, b = sweep(off, 0, w)
        if k >= WARM:
            t_on.append(a_ms); t_off.append(b_ms)
        same = same and all(torch.equal(a[key], b[key]) for key in ("z", "status", "pivots", "active", "resid"))
        solved = solved and bool((a["status"] == 1).all())
    eng.set_option(OPT_CRASH_CACHE_BIG, 1)
    info = on.info()
    refill = []
    for k in range(FILLS):
        on.update("Ad", rec[3])
        assert not on.info()["big_cached"]
        refill.append(sweep(on, 1, ws[k])[0])
    fill = []
    for k in range(FILLS):
        fresh = eng.upload_nodes(*rec)
        fill.append(sweep(fresh, 1, ws[k])[0])
        assert fresh.info()["big_cached"]
        fresh.close()
    on.close(); off.close()
    eng.set_option(OPT_CRASH_CACHE_BIG, 0)
    med = lambda v: float(np.median(v))
    un, re_ = med(t_off), med(t_on)
    spread = max(t_off) - min(t_off)
    print(f"{tag}: {NODES} x ({n}, {m}, {p}){' asymmetric Qd' if asym else ''}; {SWEEPS} sweeps after {WARM}; cache installed {info['big_cached']}; "
          f"outputs identical {same}; all solved {solved}")
    print(f"  uncached {un:8.3f} ms   (min {min(t_off):.3f}, max {max(t_off):.3f}, max - min {spread:.3f})")
    print(f"  reuse    {re_:8.3f} ms   (min {min(t_on):.3f}, max {max(t_on):.3f})   uncached - reuse = {un - re_:.3f} ms = {100 * (un - re_) / un:.1f} %; "
          f"{'beyond' if un - re_ > spread else 'WITHIN'} the uncached sweep's spread")
    gain = [b_ - a_ for a_, b_ in zip(t_on, t_off)]
    print(f"  pairwise (the same w on both handles): uncached - reuse min {min(gain):.3f}, median {med(gain):.3f}, max {max(gain):.3f} ms; "
          f"reuse faster in {sum(g > 0 for g in gain)} of {len(gain)} pairs")
    print(f"  fill     {med(fill):8.3f} ms   (fresh handles, with the allocation: {', '.join(f'{v:.3f}' for v in fill)})")
    print(f"  refill   {med(refill):8.3f} ms   (cache dropped, memory kept: {', '.join(f'{v:.3f}' for v in refill)}); over an uncached sweep: {med(refill) - un:+.3f} ms",
          flush=True)


shapes = dict(sym=(256, 256, 8, False), asym=(256, 256, 8, True), small=(144, 16, 8, False))
for c in cases:
    run(c, *shapes[c])
