"""Warm start of the mid-size classes (Nodes.set_warm, csrc/qpn_warm_mid.hip): accepted share, the share the LDS rule turns away
and time per sweep, cold against warm on the same handle.

tools/warm_rate.py's protocol, per shape: resident records of synthetic.synth_nodes on ONE handle that has opted in.  A run is a
walk of the shared parameter vector: every sweep moves every entry of w by the relative step delta, w_i <- w_i (1 + delta s_i)
with random signs s_i.  At each w of the walk the cold sweep (no hint) and the warm sweep (hint = the z the previous warm sweep
left, in place) are timed one after the other -- host clock around a synchronise --, after `--warmup` untimed steps.  The lines
give every measurement, the medians, the share of the nodes that came back with pivots = 0 (for the cold sweep: the nodes without
an active row, which need no pivot anyway) and the share of the hints that level_batch.warm_mid_fits does not admit.

    python tools/warm_mid_rate.py [--shapes 4096x48x48 4096x64x64 1024x97x64 1024x96x96 1024x128x128] [--rounds 40] [--warmup 8]
                                  [--deltas 0 1e-3 1e-1]
"""
import argparse

import numpy as np

import rate_common as RC
from qpn_amd import level_batch, synthetic
from qpn_amd.engine import colmajor


def run_shape(eng, nodes, n, m, args):
    import torch
    p = 8
    Q, R, qd, A, B, l, u = synthetic.synth_nodes(0, nodes, n, m, p)
    rec = RC.on_device(eng, (colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u))
    h = eng.upload_nodes(*rec)
    h.set_warm(True)
    w0 = synthetic.shared_params(p)
    info = dict(nodes=nodes, n=n, m=m)
    admitted = torch.tensor([level_batch.warm_mid_fits(n, k) for k in range(m + 1)], device="cuda")
    for delta in args.deltas:
        rng = np.random.default_rng(17)
        steps = args.warmup + args.rounds
        walk = w0[None, :] * np.cumprod(1.0 + delta * rng.choice([-1.0, 1.0], size=(steps + 1, p)), axis=0)
        ring, = RC.on_device(eng, (walk,))
        cold = h.solve(ring[0])
        warm = h.solve(ring[0])
        assert bool((cold["status"] == 1).all()), "the cold sweep does not solve every node"
        times = {"cold": [], "warm": []}
        shares = {"cold": [], "warm": [], "unfit": []}
        for t in range(1, steps + 1):
            w = ring[t]
            unfit = float((~admitted[(warm["z"][:, n:] != 0).sum(dim=1)]).double().mean())      # of the hint about to go in
            s_cold = RC.timed(lambda: h.solve(w, out=cold))
            s_warm = RC.timed(lambda: h.solve(w, out=warm, warm=warm["z"]))
            ok = bool((warm["status"] == 1).all()) and bool((cold["status"] == 1).all())
            zero = {"cold": float((cold["pivots"] == 0).double().mean()), "warm": float((warm["pivots"] == 0).double().mean())}
            dz = float((warm["z"] - cold["z"]).abs().max())
            if t > args.warmup:
                shares["unfit"].append(unfit)
                for k, s in (("cold", s_cold), ("warm", s_warm)):
                    times[k].append(s); shares[k].append(zero[k])
                    RC.emit(what="warm_mid_rate", delta=delta, sweep=k, round=t - args.warmup - 1, ms=s * 1e3, zero_pivot_share=zero[k],
                            unfit_share=unfit, all_solved=ok, max_abs_dz=dz, **info)
        RC.emit(what="warm_mid_rate", delta=delta, median_ms={k: float(np.median(v)) * 1e3 for k, v in times.items()},
                median_zero_pivot_share={k: float(np.median(shares[k])) for k in ("cold", "warm")},
                median_unfit_share=float(np.median(shares["unfit"])), rounds=args.rounds, warmup=args.warmup, **info)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x48x48", "4096x64x64", "1024x97x64", "1024x96x96", "1024x128x128"])
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--deltas", type=float, nargs="+", default=[0.0, 1e-3, 1e-1])
    args = ap.parse_args()
    eng = RC.qpn_amd.default_engine(0)
    for shape in args.shapes:
        nodes, n, m = (int(v) for v in shape.split("x"))
        run_shape(eng, nodes, n, m, args)


if __name__ == "__main__":
    main()
