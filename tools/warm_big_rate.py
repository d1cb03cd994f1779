#!/usr/bin/env python3
"""Developer aid: what a sweep over resident LARGE symmetric records costs with and without the warm start of block principal
pivoting (QPN_OPT_WARM_BIG with QPN_AVI_FLAG_WARM_DUALS).  The same records go on two handles in one process;
w walks by a relative delta per entry and sweep, and at every w the un-hinted sweep (one handle, cold) and the hinted sweep (the
other handle: the z of its previous hinted sweep goes in as the hint, in place) run one after the other, each between two
synchronisations under a host clock.  Per case, crash-cache setting (QPN_OPT_CRASH_CACHE_BIG) and delta: medians, min ... max,
the pairwise differences at the same w, the share of hinted nodes with pivots == n ("the hint held"), the mean number of
complementarity pairs switched, and whether every node solved.  THE CLAIM (as in 5q): at the same w the hinted sweep is faster
than the un-hinted one in every pair, by more than the un-hinted sweep's own max - min.
Cases: c5 = config 5's records (512 x (256, 256, 8)), small = 512 x (144, 16, 8).
Usage: python tools/warm_big_rate.py [c5] [small]   (NODES=512 WARM=8 SWEEPS=40 CACHE="0 1" DELTAS="0 1e-3 1e-1")"""
import os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np, torch
import qpn_amd
import problems as P
from qpn_amd.engine import colmajor
from qpn_amd._lib import OPT_CRASH_CACHE_BIG, OPT_WARM_BIG

cases = sys.argv[1:] or ["c5", "small"]
NODES = int(os.environ.get("NODES", "512")); WARM = int(os.environ.get("WARM", "8")); SWEEPS = int(os.environ.get("SWEEPS", "40"))
CACHE = [int(v) for v in os.environ.get("CACHE", "0 1").split()]
DELTAS = [float(v) for v in os.environ.get("DELTAS", "0 1e-3 1e-1").split()]
eng = qpn_amd.Engine(0)
eng.set_option(OPT_WARM_BIG, 1)
t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def timed(call):
    torch.cuda.synchronize(); eng.synchronize()
    t0 = time.perf_counter()
    res = call()
    torch.cuda.synchronize(); eng.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def run(tag, n, m, p, rec, cache, delta):
    eng.set_option(OPT_CRASH_CACHE_BIG, cache)
    rng = np.random.default_rng(1)
    w = rng.standard_normal(p)
    cold, hot = eng.upload_nodes(*rec), eng.upload_nodes(*rec)
    out_c = cold.solve(t(w))
    out_h = hot.solve(t(w))                                  # the first hint: this handle's own cold solution
    t_c, t_h, held, sw_c, sw_h, solved = [], [], [], [], [], True
    for k in range(WARM + SWEEPS):
        w = w * (1.0 + delta * rng.standard_normal(p))
        wd = t(w)
        c_ms, _ = timed(lambda: cold.solve(wd, out=out_c))
        h_ms, _ = timed(lambda: hot.solve(wd, out=out_h, warm=out_h["z"]))
        solved = solved and bool((out_c["status"] == 1).all()) and bool((out_h["status"] == 1).all())
        if k >= WARM:
            t_c.append(c_ms); t_h.append(h_ms)
            held.append(float((out_h["pivots"] == n).double().mean()))
            sw_c.append(float((out_c["pivots"] - n).double().mean())); sw_h.append(float((out_h["pivots"] - n).double().mean()))
    dz = float((out_c["z"] - out_h["z"]).abs().max())
    info = hot.info()
    cold.close(); hot.close()
    med = lambda v: float(np.median(v))
    spread = max(t_c) - min(t_c)
    gain = [a - b for a, b in zip(t_c, t_h)]
    claim = min(gain) > spread
    print(f"{tag}: {NODES} x ({n}, {m}, {p}); crash cache {cache} (installed {info['big_cached']}); delta {delta:g}; {SWEEPS} sweeps after {WARM}; "
          f"all solved {solved}; last sweep max |z_hinted - z_unhinted| {dz:.2e}")
    print(f"  un-hinted {med(t_c):8.3f} ms   (min {min(t_c):.3f}, max {max(t_c):.3f}, max - min {spread:.3f}); mean pairs switched {np.mean(sw_c):.1f}")
    print(f"  hinted    {med(t_h):8.3f} ms   (min {min(t_h):.3f}, max {max(t_h):.3f}); mean pairs switched {np.mean(sw_h):.2f}; "
          f"nodes with pivots == n {100 * np.mean(held):.1f} %")
    print(f"  pairwise (the same w): un-hinted - hinted min {min(gain):.3f}, median {med(gain):.3f}, max {max(gain):.3f} ms; hinted faster in "
          f"{sum(g > 0 for g in gain)} of {len(gain)} pairs; the claim (every pair, by more than {spread:.3f} ms) {'HOLDS' if claim else 'does NOT hold'}",
          flush=True)


shapes = dict(c5=(256, 256, 8), small=(144, 16, 8))
for c in cases:
    n, m, p = shapes[c]
    Q, R_, qd, A, B, l, u = P.synth_nodes(0, NODES, n, m, p)
    rec = [t(colmajor(Q)), t(colmajor(R_)), t(qd), t(colmajor(A)), t(colmajor(B)), t(l), t(u)]
    for cache in CACHE:
        for delta in DELTAS:
            run(c, n, m, p, rec, cache, delta)
eng.set_option(OPT_CRASH_CACHE_BIG, 0)
eng.set_option(OPT_WARM_BIG, 0)
