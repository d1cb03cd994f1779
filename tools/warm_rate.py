"""Warm start of the 32-class node sweep (QPN_AVI_FLAG_WARM_DUALS): accepted share and time per sweep, flag off against flag on.

Resident records of synthetic.synth_nodes at `--nodes` x (32, 32) on one handle.  A run is a walk of the shared parameter
vector: every sweep moves every entry of w by the relative step delta, w_i <- w_i (1 + delta s_i) with random signs s_i.  At
each w of the walk the cold sweep (flag off) and the warm sweep (flag on, hint = the z the previous warm sweep left, in place)
are timed one after the other -- host clock around a synchronise --, after `--warmup` untimed steps; the lines give every
measurement, the medians, and the share of the nodes that came back with pivots = 0 (for the cold sweep: the nodes without an
active row, which need no pivot anyway).

    python tools/warm_rate.py [--nodes 10000] [--rounds 40] [--warmup 8] [--deltas 0 1e-3 1e-1]
"""
import argparse

import numpy as np

import rate_common as RC
from qpn_amd import synthetic
from qpn_amd.engine import colmajor


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--deltas", type=float, nargs="+", default=[0.0, 1e-3, 1e-1])
    args = ap.parse_args()
    n = m = 32
    p = 8
    eng = RC.qpn_amd.default_engine(0)
    Q, R, qd, A, B, l, u = synthetic.synth_nodes(0, args.nodes, n, m, p)
    rec = RC.on_device(eng, (colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u))
    h = eng.upload_nodes(*rec)
    w0 = synthetic.shared_params(p)
    info = dict(nodes=args.nodes, n=n, m=m)
    for delta in args.deltas:
        rng = np.random.default_rng(17)
        steps = args.warmup + args.rounds
        walk = w0[None, :] * np.cumprod(1.0 + delta * rng.choice([-1.0, 1.0], size=(steps + 1, p)), axis=0)
        ring, = RC.on_device(eng, (walk,))
        cold = h.solve(ring[0])
        warm = h.solve(ring[0])
        assert bool((cold["status"] == 1).all()), "the cold sweep does not solve every node"
        times = {"off": [], "on": []}
        shares = {"off": [], "on": []}
        for t in range(1, steps + 1):
            w = ring[t]
            s_off = RC.timed(lambda: h.solve(w, out=cold))
            s_on = RC.timed(lambda: h.solve(w, out=warm, warm=warm["z"]))
            ok = bool((warm["status"] == 1).all()) and bool((cold["status"] == 1).all())
            zero = {"off": float((cold["pivots"] == 0).double().mean()), "on": float((warm["pivots"] == 0).double().mean())}
            dz = float((warm["z"] - cold["z"]).abs().max())
            if t > args.warmup:
                for k, s in (("off", s_off), ("on", s_on)):
                    times[k].append(s); shares[k].append(zero[k])
                    RC.emit(what="warm_rate", delta=delta, flag=k, round=t - args.warmup - 1, ms=s * 1e3, zero_pivot_share=zero[k],
                            all_solved=ok, max_abs_dz=dz, **info)
        RC.emit(what="warm_rate", delta=delta, median_ms={k: float(np.median(v)) * 1e3 for k, v in times.items()},
                median_zero_pivot_share={k: float(np.median(v)) for k, v in shares.items()}, rounds=args.rounds, warmup=args.warmup,
                **info)
    h.close()


if __name__ == "__main__":
    main()
