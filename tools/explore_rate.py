"""Rates of multiplier-vertex exploration: qpn_multiplier_vertices on batches of degenerate multiplier
sets -- config-2-shaped items (n = 2, m = 5 .. 12) and synthetic LP followers (n = 3 .. 32, m up to 64) -- and the extra wall
time of solve() on config 2 (robust_avoid_simple) with exploration_vertices = 10 over the default.

    python tools/explore_rate.py [--batch 2000] [--reps 5] [--out FILE]

Times are host wall clock around calls on device buffers that end in a synchronise (median of --reps after one warm-up)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import qpn_amd  # noqa: E402
from qpn_amd import algorithm, examples  # noqa: E402
from exploration_cases import degenerate_case  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    eng = qpn_amd.default_engine(0)
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"# qpn_multiplier_vertices, V = 10 (basis budget 640), batch {a.batch}, device buffers")
    say("n m kind ms_per_batch us_per_item mean_vertices statuses(complete,vbudget,bbudget,empty,novertex)")
    for n, m, kind in [(2, 5, "mixed"), (2, 12, "mixed"), (3, 6, "lp"), (8, 16, "lp"), (16, 32, "lp"), (32, 32, "lp"),
                       (16, 64, "lp"), (32, 64, "lp")]:
        rng = np.random.default_rng(n * 100 + m)
        cs = [degenerate_case(rng, n, m, kind) for _ in range(a.batch)]
        to = lambda k, dt=torch.float64: torch.as_tensor(np.stack([c[k] for c in cs]), dtype=dt, device="cuda:0")
        Ac, g, cls, lam = to(0), to(1), to(2, torch.uint8), to(3)
        eng.multiplier_vertices(Ac, g, cls, lam, 10)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            v, c, s = eng.multiplier_vertices(Ac, g, cls, lam, 10)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(ts))
        st = np.bincount(s.cpu().numpy(), minlength=5)
        say(f"{n} {m} {kind} {ms:.3f} {1e3 * ms / a.batch:.3f} {float(c.float().mean()):.2f} {tuple(int(x) for x in st)}")
    say("# solve() on config 2 (robust_avoid_simple, num_projections = 5): wall seconds, default vs exploration_vertices = 10")
    for seed in (1, 2, 3):
        row = []
        for E in (0, 10):
            algorithm.solve(examples.setup("robust_avoid_simple", seed=seed, num_projections=5, exploration_vertices=E), engine=eng)
            t0 = time.perf_counter()
            r = algorithm.solve(examples.setup("robust_avoid_simple", seed=seed, num_projections=5, exploration_vertices=E), engine=eng)
            row.append((time.perf_counter() - t0, r["solved"]))
        say(f"seed {seed}: E=0 {row[0][0]:.3f} s solved={row[0][1]}  E=10 {row[1][0]:.3f} s solved={row[1][1]}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
