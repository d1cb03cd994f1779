"""Rate of qpn_convexity_nodes (csrc/qpn_convexity.hip) on device-resident inputs, and the cost of
QPNetOptions.check_convexity on a whole solve().

    python tools/convexity_rate.py [--reps 20] [--pairs 200]

Shapes: 10 000 x (n, m) = (32, 32) (the wave class) and 512 x (256, 256) (the global-workspace class), half of the rows
marked as implicit equalities.  Kernel time from HIP events around `reps` back-to-back calls after a warm-up call; solve()
time is wall time of one solve per setting after a warm-up solve."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_rate(eng, batch, n, m, reps):
    import torch
    g = np.random.Generator(np.random.Philox(key=[11, n]))
    G = g.standard_normal((batch, n, n))
    Qc = torch.tensor(G @ np.swapaxes(G, 1, 2) / n - 0.1 * np.eye(n), device="cuda:0")
    Ac = torch.tensor(g.standard_normal((batch, n, m)), device="cuda:0")
    eq = torch.tensor((g.random((batch, m)) < 0.5).astype(np.uint8), device="cuda:0")
    eng.convexity_nodes(Qc, Ac, eq)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        cvx, lam, nd = eng.convexity_nodes(Qc, Ac, eq)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / reps
    return dict(batch=batch, n=n, m=m, ms_per_call=ms, nodes_per_s=batch / (ms * 1e-3),
                input_mb=(Qc.numel() + Ac.numel()) * 8 / 1e6 + eq.numel() / 1e6,
                null_dim_mean=float(nd.double().mean()), convex_share=float(cvx.double().mean()))


def solve_cost(eng, pairs):
    from qpn_amd import algorithm, examples
    out = {}
    for on in (False, True):
        algorithm.solve(examples.setup("synthetic_pairs", pairs=pairs, n=16, m=16, check_convexity=on), engine=eng)
        before = dict(eng.seconds)
        t = time.perf_counter()
        r = algorithm.solve(examples.setup("synthetic_pairs", pairs=pairs, n=16, m=16, check_convexity=on), engine=eng)
        wall = time.perf_counter() - t
        spent = {k: v - before.get(k, 0.0) for k, v in eng.seconds.items() if v - before.get(k, 0.0) > 1e-3}
        out["on" if on else "off"] = dict(seconds=wall, solved=bool(r["solved"]), library_seconds=spent)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=200)
    a = ap.parse_args()
    import qpn_amd
    eng = qpn_amd.default_engine(0)
    res = dict(kernel=[kernel_rate(eng, 10000, 32, 32, a.reps), kernel_rate(eng, 512, 256, 256, max(1, a.reps // 4))])
    res["solve"] = solve_cost(eng, a.pairs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
