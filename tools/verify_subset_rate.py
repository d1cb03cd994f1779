"""The accept gate over a part of a resident handle (qpn_verify_nodes_subset_h): time per call against the count of listed nodes,
beside the full call of the same handle on the same build.

Resident records of synthetic.synth_nodes at `--nodes` x (n, m) on one handle, one w row per node, xd the solved point of every
node (all nodes optimal: the least-squares path).  A group times `--calls` back-to-back calls of every route between two
synchronisations -- host clock, us per call --, the routes alternating inside the group: the full call (Nodes.verify) and
Nodes.verify_subset at every `--counts` entry over a fixed random list of that many nodes (a count equal to `--nodes` lists
every node: the cost of the list itself).  `--mem host` passes numpy arrays (idx, xd and w up and the outputs down over PCIe
inside every call).  The last line gives the medians over the groups.  With `--full-only` the subset routes are left out: a copy
of this file run that way inside another checkout (the parent commit's tree and build) gives that build's full call taken the
same way.

    python tools/verify_subset_rate.py [--n 32 --m 32] [--nodes 10000] [--counts 10000 1000 100 10] [--mem device] [--full-only]
"""
import argparse

import numpy as np

import rate_common as RC
from qpn_amd import synthetic
from qpn_amd.engine import colmajor


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--counts", type=int, nargs="+", default=[10_000, 1_000, 100, 10])
    ap.add_argument("--groups", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mem", choices=("device", "host"), default="device")
    ap.add_argument("--full-only", action="store_true")
    args = ap.parse_args()
    n, m, p, batch = args.n, args.m, 8, args.nodes
    dev = args.mem == "device"
    eng = RC.qpn_amd.default_engine(0)
    Q, R, qd, A, B, l, u = synthetic.synth_nodes(0, batch, n, m, p)
    h = eng.upload_nodes(*RC.on_device(eng, (colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u)))
    rng = np.random.default_rng(29)
    w_host = synthetic.shared_params(p)[None, :] + 0.05 * rng.standard_normal((batch, p))
    put = (lambda a: RC.on_device(eng, (a,))[0]) if dev else (lambda a: np.ascontiguousarray(a))
    host = lambda a: np.asarray(a.cpu() if dev else a)
    x_host = np.ascontiguousarray(host(h.solve(put(w_host), want=("z",))["z"])[:, :n])
    xd, w = put(x_host), put(w_host)
    full = [host(a) for a in h.verify(xd, w)]
    eng.synchronize()
    info = dict(n=n, m=m, nodes=batch, mem=args.mem, calls=args.calls, optimal=int(full[0].sum()),
                paths=np.bincount(full[2], minlength=7).tolist())
    routes = [("full", lambda: h.verify(xd, w))]
    if not args.full_only:
        for count in args.counts:
            count = min(count, batch)
            idx_host = np.sort(rng.permutation(batch)[:count]).astype(np.int32)
            idx, xs, ws = put(idx_host), put(x_host[idx_host]), put(w_host[idx_host])
            got = [host(a) for a in h.verify_subset(idx, xs, ws)]
            assert all(np.array_equal(g, f[idx_host]) for g, f in zip(got, full)), "the subset call's answers are not the full call's"
            routes.append((f"subset_{count}", lambda idx=idx, xs=xs, ws=ws: h.verify_subset(idx, xs, ws)))
    times = {name: [] for name, _ in routes}
    for g in range(args.warmup + args.groups):
        for name, fn in routes:
            s = RC.timed(lambda: [fn() for _ in range(args.calls)]) / args.calls
            if g >= args.warmup:
                times[name].append(s)
                RC.emit(what="verify_subset_rate", route=name, group=g - args.warmup, us_per_call=s * 1e6, n=n, m=m, nodes=batch, mem=args.mem)
    RC.emit(what="verify_subset_rate", median_us_per_call={k: float(np.median(v)) * 1e6 for k, v in times.items()},
            min_us_per_call={k: float(np.min(v)) * 1e6 for k, v in times.items()}, groups=args.groups, **info)
    h.close()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
